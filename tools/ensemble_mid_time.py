"""What the ensembles' workspace tier costs: M copies of a 2-D journal bearing (50 x 50 and 100 x 100, the reference's mass
conservation and flip symmetry set-ups at U = 10 m/s), 200 steps per member and call, honor_stop off.

For every shape and M two legs in one process, interleaved, REPEATS times each:
  (a) one Ensemble._advance of M members                  one launch of k_mid_ensemble, one workgroup per member
  (b) the same M members, Problem._advance one after another      k_step2, one member at a time (what a sweep cost before)
Both legs are wall times of the Python calls, the copy of the per-step records and the host's bookkeeping included.  Reports
median and spread (min .. max) per leg as us per member-step, and their ratio.

    python tools/ensemble_mid_time.py [--out DIR]

Writes DIR/ensemble_mid_time.json (default profiles/ensemble_mid)."""
import contextlib
import io
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gapflow_amd import Ensemble, Problem  # noqa: E402
from gapflow_amd import _lib  # noqa: E402

T = """
options: {{silent: True}}
grid: {{Nx: {n}, Ny: {n}, dx: 2.e-5, dy: 2.e-5}}
geometry: {{type: journal, CR: 1.e-2, eps: 0.7, U: 10., V: 0.}}
numerics: {{CFL: 0.5, adaptive: 1, tol: 1.e-30, max_it: 100000000}}
properties: {{EOS: DH, shear: 0.0794, bulk: 0., rho0: 877.7007, P0: 101325., C1: 3.5e10, C2: 1.23}}
"""
SHAPES = (50, 100)
MS = (1, 16, 64, 256, 512)
STEPS, REPEATS = 200, 3


def main():
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join('profiles', 'ensemble_mid')
    os.makedirs(out, exist_ok=True)
    _lib.require_device()
    shapes = []
    for n in SHAPES:
        with contextlib.redirect_stdout(io.StringIO()):
            ps = [Problem.from_string(T.format(n=n)) for _ in range(max(MS))]
            for p in ps:
                p._pre_run()

        def solo(m):
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                for p in ps[:m]:
                    p._advance(STEPS, honor_stop=False)
            return time.perf_counter() - t0

        results = []
        for m in MS:
            ens = Ensemble(ps[:m])
            assert set(ens.tiers) == {'workspace'}

            def together():
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    ens._advance([STEPS] * m, honor_stop=False)
                return time.perf_counter() - t0

            solo(min(m, 4))                     # warm both paths (code objects) outside the timing
            together()
            ta, tb = [], []
            for _ in range(REPEATS):            # interleaved: drift of the clocks hits both legs alike
                ta.append(together())
                tb.append(solo(m))
            del ens
            results.append({'M': m, 'steps': STEPS, 'repeats': REPEATS, 'ensemble_s': ta, 'solo_s': tb})
            a, b = statistics.median(ta), statistics.median(tb)
            line = f"{n:3d} x {n:<3d} M={m:4d}"
            for name, ts, med in (('ensemble', ta, a), ('one after another', tb, b)):
                line += (f"  {name}: {med / (m * STEPS) * 1e6:8.3f} us/member-step ({min(ts) / (m * STEPS) * 1e6:.3f} .. "
                         f"{max(ts) / (m * STEPS) * 1e6:.3f})")
            print(line + f"  ensemble step {a / STEPS * 1e6:8.1f} us  ratio {b / a:6.2f}x", flush=True)
        # a run that went invalid would return at once and time nothing: every member must have taken every step asked of it
        for k in (0, max(MS) - 1):
            print(f"{n} x {n} member {k}: step {ps[k].step}, stopped {ps[k]._stop}")
            assert not ps[k]._stop and ps[k].step % STEPS == 0 and ps[k].step > 0
        shapes.append({'Nx': n, 'Ny': n, 'results': results})
        del ps
    with open(os.path.join(out, 'ensemble_mid_time.json'), 'w') as f:
        json.dump({'lib': os.environ.get('GPF_LIB_PATH', 'default'), 'shapes': shapes}, f, indent=1)


if __name__ == '__main__':
    main()
