"""What recording film integrals costs on the one-workgroup kernels, honor_stop off, REPEATS wall-clock timings per leg.

  (a) solo: the 1-D journal bearing of tools/ensemble_time.py (100 x 1), 2000 steps per gpf_step call, integrals armed at
      every = 1, and the same call with nothing armed.  ms per step.
  (b) ensembles: 256 members of that problem, and 16 members of a 50 x 50 journal bearing (workspace tier), 2000 / 200 steps per
      gpf_ensemble_step, with and without gpf_ensemble_integrals_set(every = 1); the legs interleaved.  us per member-step and
      the difference, the cost of recording.

    python tools/ensemble_integrals_time.py [--out DIR] [--solo-only]

--solo-only runs (a) alone and asks the library for none of the entry points this measurement is about, so it also runs on a
library built from an earlier commit (GPF_LIB_PATH): there every = 1 is the batch cut at every step, the baseline.
Writes DIR/ensemble_integrals_time[.solo].json (default profiles/ensemble_integrals)."""
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

ONE_D = """
options: {silent: True}
grid: {Nx: 100, Ny: 1, dx: 1.e-5, dy: 1.}
geometry: {type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.}
numerics: {CFL: 0.25, adaptive: 1, tol: 1.e-30, max_it: 100000000}
properties: {EOS: DH, shear: 0.0794, bulk: 0., rho0: 877.7007}
"""
TWO_D = ONE_D.replace('Nx: 100, Ny: 1, dx: 1.e-5, dy: 1.', 'Nx: 50, Ny: 50, Lx: 0.1, Ly: 0.02').replace('U: 0.1', 'U: 10.')
REPEATS = 5
NEW = ('gpf_ensemble_integrals_set', 'gpf_ensemble_integrals_clear', 'gpf_ensemble_integrals_read', 'gpf_integrals_in_batch')


def problems(text, m):
    with contextlib.redirect_stdout(io.StringIO()):
        ps = [Problem.from_string(text) for _ in range(m)]
        for p in ps:
            p._pre_run()
    return ps


def spread(ts, per):
    return dict(median=statistics.median(ts) / per, min=min(ts) / per, max=max(ts) / per)


def solo(lib, steps=2000):
    p = problems(ONE_D, 1)[0]
    nexec = C.c_int64(0)

    def call():
        t0 = time.perf_counter()
        _lib.check(lib.gpf_step(p._h, steps, 0, None, 0, C.byref(nexec)))
        return time.perf_counter() - t0

    out = {}
    for name in ('unarmed', 'every1'):
        if name == 'every1':
            _lib.check(lib.gpf_integrals_set(p._h, 1, 0, None, 0, None))
        call()                                  # warm: code objects, buffers
        ts = [call() for _ in range(REPEATS)]
        out[name] = dict(seconds=ts, ms_per_step=spread(ts, steps / 1e3))
        s = out[name]['ms_per_step']
        print(f"solo 100 x 1, {name:8s}: {s['median']:.5f} ms/step ({s['min']:.5f} .. {s['max']:.5f})", flush=True)
    have = C.c_int64(0)
    _lib.check(lib.gpf_integrals_read(p._h, None, 0, None, C.byref(have)))
    sc = _lib.GpfScalars()
    _lib.check(lib.gpf_state(p._h, C.byref(sc)))
    assert have.value == steps and sc.invalid == 0 and sc.step == 2 * (REPEATS + 1) * steps, (have.value, sc.step, sc.invalid)
    return out


def ensemble(lib, text, m, steps, label):
    ps = problems(text, m)
    handles = (C.c_void_p * m)(*[p._h.value for p in ps])
    n, done = (C.c_int64 * m)(*([steps] * m)), (C.c_int64 * m)()
    e = C.c_void_p()
    _lib.check(lib.gpf_ensemble_create(handles, m, C.byref(e)))

    def call(armed):
        if armed:
            _lib.check(lib.gpf_ensemble_integrals_set(e, 1, 0, None, 0, None))
        else:
            _lib.check(lib.gpf_ensemble_integrals_clear(e))
        t0 = time.perf_counter()
        _lib.check(lib.gpf_ensemble_step(e, n, 0, done))
        return time.perf_counter() - t0

    call(False), call(True)                     # warm both
    plain, armed = [], []
    for _ in range(REPEATS):                    # interleaved: drift hits both legs alike
        plain.append(call(False))
        armed.append(call(True))
    have = C.c_int64(0)
    _lib.check(lib.gpf_ensemble_integrals_read(e, m - 1, None, 0, None, C.byref(have)))
    assert have.value == steps and all(d == (2 * REPEATS + 2) * steps for d in done), (have.value, done[0])
    _lib.check(lib.gpf_ensemble_destroy(e))
    per = m * steps / 1e6
    a, b = spread(plain, per), spread(armed, per)
    print(f"{label}: {m} members x {steps} steps: unarmed {a['median']:.4f} us/member-step ({a['min']:.4f} .. {a['max']:.4f}), "
          f"every = 1 {b['median']:.4f} ({b['min']:.4f} .. {b['max']:.4f}), recording {b['median'] - a['median']:.4f}", flush=True)
    return dict(members=m, steps=steps, unarmed_s=plain, armed_s=armed, unarmed_us=a, armed_us=b, recording_us=b['median'] - a['median'])


def main():
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join('profiles', 'ensemble_integrals')
    solo_only = '--solo-only' in sys.argv
    os.makedirs(out, exist_ok=True)
    if solo_only:
        for name in NEW:
            _lib.SIGNATURES.pop(name, None)
    lib = _lib.require_device()
    res = {'lib': os.path.basename(os.environ.get('GPF_LIB_PATH', 'default')), 'repeats': REPEATS, 'solo_100x1': solo(lib)}
    if not solo_only:
        res['ensemble_256_of_100x1'] = ensemble(lib, ONE_D, 256, 2000, 'LDS tier, 100 x 1')
        res['ensemble_16_of_50x50'] = ensemble(lib, TWO_D, 16, 200, 'workspace tier, 50 x 50')
    with open(os.path.join(out, 'ensemble_integrals_time.solo.json' if solo_only else 'ensemble_integrals_time.json'), 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
