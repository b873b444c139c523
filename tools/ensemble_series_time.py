"""What the ensembles' extrema series and point probes cost inside the one-workgroup kernels, honor_stop off, wall clock per
gpf_ensemble_step.

Three configurations: 256 members of the 1-D journal bearing of tools/ensemble_time.py (100 x 1, LDS tier, 2000 steps per call),
16 members of a 50 x 50 and 16 of a 100 x 100 journal bearing (workspace tier, 200 / 100 steps per call).  Per configuration three
legs, interleaved so that drift hits them alike, REPEATS timings each: nothing armed, gpf_ensemble_extrema_set(every = 1), and 8
probes with p (gpf_ensemble_probes_set).  us per member-step, and the difference to the unarmed leg: the cost of a record.

    python tools/ensemble_series_time.py [--out DIR] [--unarmed-only] [--tag NAME]

--unarmed-only times the first leg alone and asks the library for none of the entry points this measurement is about, so it also
runs on a library built from an earlier commit (GPF_LIB_PATH): alternate the two libraries, process by process, to compare them.
A library built with -DGPF_MID_EXTREMA_PER_WAVE (python -m gapflow_amd.build --variant perwave -DGPF_MID_EXTREMA_PER_WAVE) records
the workspace tier's extrema with the LDS tier's one wave per quantity: run it under GPF_LIB_PATH for that comparison.
Writes DIR/ensemble_series_time[.TAG].json (default profiles/ensemble_series)."""
import contextlib
import ctypes as C
import io
import json
import os
import statistics
import sys
import time

import numpy as np

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


def two_d(n):
    return ONE_D.replace('Nx: 100, Ny: 1, dx: 1.e-5, dy: 1.', f'Nx: {n}, Ny: {n}, Lx: 0.1, Ly: 0.02').replace('U: 0.1', 'U: 10.')


REPEATS = 5
NEW = ('gpf_ensemble_extrema_set', 'gpf_ensemble_extrema_clear', 'gpf_ensemble_extrema_read', 'gpf_ensemble_probes_set',
       'gpf_ensemble_probes_clear', 'gpf_ensemble_probes_read')
CONFIGS = (('ensemble_256_of_100x1', ONE_D, 256, 2000, 100, 1), ('ensemble_16_of_50x50', two_d(50), 16, 200, 50, 50),
           ('ensemble_16_of_100x100', two_d(100), 16, 100, 100, 100))


def problems(text, m):
    with contextlib.redirect_stdout(io.StringIO()):
        ps = [Problem.from_string(text) for _ in range(m)]
        for p in ps:
            p._pre_run()
    return ps


def spread(ts, per):
    return dict(median=statistics.median(ts) / per, min=min(ts) / per, max=max(ts) / per)


def ensemble(lib, label, text, m, steps, nx, ny, legs):
    ps = problems(text, m)
    handles = (C.c_void_p * m)(*[p._h.value for p in ps])
    n, done = (C.c_int64 * m)(*([steps] * m)), (C.c_int64 * m)()
    e = C.c_void_p()
    _lib.check(lib.gpf_ensemble_create(handles, m, C.byref(e)))
    i32 = C.POINTER(C.c_int32)
    count = np.array([8], dtype=np.int32)
    cells = np.array([[1 + (k * nx) // 8, 1 + (k * ny) // 8] for k in range(8)], dtype=np.int32)        # along the diagonal

    def call(leg):
        if leg == 'extrema':
            _lib.check(lib.gpf_ensemble_extrema_set(e, 1))
        elif leg == 'probes':
            _lib.check(lib.gpf_ensemble_probes_set(e, 0, count.ctypes.data_as(i32), cells.ctypes.data_as(i32), 1))
        t0 = time.perf_counter()
        _lib.check(lib.gpf_ensemble_step(e, n, 0, done))
        dt = time.perf_counter() - t0
        have = C.c_int64(0)
        if leg == 'extrema':
            _lib.check(lib.gpf_ensemble_extrema_read(e, m - 1, None, None, 0, None, C.byref(have)))
            _lib.check(lib.gpf_ensemble_extrema_clear(e))
        elif leg == 'probes':
            _lib.check(lib.gpf_ensemble_probes_read(e, m - 1, None, 0, None, C.byref(have)))
            _lib.check(lib.gpf_ensemble_probes_clear(e))
        assert leg == 'unarmed' or have.value == steps, (leg, have.value)
        return dt

    for leg in legs:
        call(leg)                               # warm: code objects, buffers
    ts = {leg: [] for leg in legs}
    for _ in range(REPEATS):                    # interleaved: drift hits all legs alike
        for leg in legs:
            ts[leg].append(call(leg))
    assert all(d == (REPEATS + 1) * len(legs) * steps for d in done), done[0]
    _lib.check(lib.gpf_ensemble_destroy(e))
    per = m * steps / 1e6
    res = dict(members=m, steps=steps, seconds=ts, us={leg: spread(ts[leg], per) for leg in legs})
    base = res['us']['unarmed']['median']
    res['recording_us'] = {leg: res['us'][leg]['median'] - base for leg in legs if leg != 'unarmed'}
    print(f"{label}: {m} members x {steps} steps, us per member-step: " +
          ', '.join(f"{leg} {s['median']:.4f} ({s['min']:.4f} .. {s['max']:.4f})" for leg, s in res['us'].items()), flush=True)
    return res


def main():
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join('profiles', 'ensemble_series')
    tag = sys.argv[sys.argv.index('--tag') + 1] if '--tag' in sys.argv else None
    unarmed_only = '--unarmed-only' in sys.argv
    os.makedirs(out, exist_ok=True)
    if unarmed_only:
        for name in NEW:
            _lib.SIGNATURES.pop(name, None)
    lib = _lib.require_device()
    legs = ('unarmed',) if unarmed_only else ('unarmed', 'extrema', 'probes')
    res = {'lib': os.path.basename(os.environ.get('GPF_LIB_PATH', 'default')), 'repeats': REPEATS}
    for label, text, m, steps, nx, ny in CONFIGS:
        res[label] = ensemble(lib, label, text, m, steps, nx, ny, legs)
    with open(os.path.join(out, f"ensemble_series_time{'.' + tag if tag else ''}.json"), 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
