"""What an ensemble costs: M copies of the 1-D journal bearing of tools/small_grid_bench.py (Nx = 100), 2000 steps per member,
honor_stop off.

For every M two legs in one process, interleaved, REPEATS times each:
  (a) one gpf_ensemble_step of M members                 wall time of the call (argument copy, launch, state copy, sync)
  (b) M solo problems advanced one after another         wall time of M gpf_step calls (no log copy either)
Reports median and spread (min .. max) per leg, as us per member-step and aggregate member-steps/s.

    python tools/ensemble_time.py [--out DIR] [--solo-only]

--solo-only runs leg (b) alone: it needs nothing of the ensemble entry points, so it also runs on a library built from an
earlier commit (GPF_LIB_PATH), which is the baseline.  Writes DIR/ensemble_time[.solo].json (default profiles/ensemble)."""
import contextlib
import ctypes as C
import io
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gapflow_amd import Problem  # noqa: E402
from gapflow_amd import _lib  # noqa: E402

T = """
options: {silent: True}
grid: {Nx: 100, Ny: 1, dx: 1.e-5, dy: 1.}
geometry: {type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.}
numerics: {CFL: 0.25, adaptive: 1, tol: 1.e-30, max_it: 100000000}
properties: {EOS: DH, shear: 0.0794, bulk: 0., rho0: 877.7007}
"""
MS = (1, 16, 64, 256, 512, 1024)
STEPS, REPEATS = 2000, 5


def main():
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join('profiles', 'ensemble')
    solo_only = '--solo-only' in sys.argv
    os.makedirs(out, exist_ok=True)
    if solo_only:       # a library built from an earlier commit has no ensemble entry points: do not ask it for them
        for name in [k for k in _lib.SIGNATURES if k.startswith('gpf_ensemble_')]:
            del _lib.SIGNATURES[name]
    lib = _lib.require_device()
    with contextlib.redirect_stdout(io.StringIO()):
        ps = [Problem.from_string(T) for _ in range(max(MS))]
        for p in ps:
            p._pre_run()
    nexec = C.c_int64(0)

    def solo(m):
        t0 = time.perf_counter()
        for p in ps[:m]:
            _lib.check(lib.gpf_step(p._h, STEPS, 0, None, 0, C.byref(nexec)))
        return time.perf_counter() - t0

    results = []
    for m in MS:
        handles = (C.c_void_p * m)(*[p._h.value for p in ps[:m]])
        n, done = (C.c_int64 * m)(*([STEPS] * m)), (C.c_int64 * m)()
        e = C.c_void_p()
        if not solo_only:
            _lib.check(lib.gpf_ensemble_create(handles, m, C.byref(e)))

        def ens():
            t0 = time.perf_counter()
            _lib.check(lib.gpf_ensemble_step(e, n, 0, done))
            return time.perf_counter() - t0

        solo(min(m, 4))                         # warm both paths (code objects, LDS attribute) outside the timing
        if not solo_only:
            ens()
        ta, tb = [], []
        for _ in range(REPEATS):                # interleaved: drift of the clocks hits both legs alike
            if not solo_only:
                ta.append(ens())
            tb.append(solo(m))
        rec = {'M': m, 'steps': STEPS, 'repeats': REPEATS, 'solo_s': tb}
        if not solo_only:
            rec['ensemble_s'] = ta
            _lib.check(lib.gpf_ensemble_destroy(e))
        results.append(rec)
        line = f"M={m:5d}"
        for name, ts in (('ensemble', ta), ('solo', tb)):
            if ts:
                med = statistics.median(ts)
                line += (f"  {name}: {med / (m * STEPS) * 1e6:8.3f} us/member-step ({min(ts) / (m * STEPS) * 1e6:.3f} .. "
                         f"{max(ts) / (m * STEPS) * 1e6:.3f}), {m * STEPS / med:12.0f} member-steps/s")
        print(line, flush=True)
    name = 'ensemble_time.solo.json' if solo_only else 'ensemble_time.json'
    with open(os.path.join(out, name), 'w') as f:
        json.dump({'lib': os.environ.get('GPF_LIB_PATH', 'default'), 'Nx': 100, 'results': results}, f, indent=1)
    # a run that went invalid would return at once and time nothing: every member must have taken every step asked of it
    sc = _lib.GpfScalars()
    for k in (0, max(MS) - 1):
        _lib.check(lib.gpf_state(ps[k]._h, C.byref(sc)))
        print(f"member {k}: step {sc.step}, invalid {sc.invalid}")
        assert sc.invalid == 0 and sc.step % STEPS == 0


if __name__ == '__main__':
    main()
