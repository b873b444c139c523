"""Time of resampling a state onto a finer grid on the device, beside a kernel that only stores the same bytes.

    python tools/resample_time.py [--src 1024] [--dst 4096] [--reps 20] [--rounds 5] [--json FILE]

One process, alternating legs, one warm-up round that is thrown away, then --rounds rounds; every figure is printed with its
median and its whole range (ms per call, HIP events on the destination's stream).  Legs (gpf_resample_time):
    resample    what gpf_resample enqueues: k_resample + the two ghost-cell kernels, --src x --src -> --dst x --dst
    store only  k_resample_store_only: the same rows, column pairs and stores of a constant, no source reads, no arithmetic
Both write the destination's buffer that does not hold its state.  The source is advanced 4 steps first, so that it is a
committed state like any other.  GPF_LIB_PATH selects another build of the library."""
import argparse
import contextlib
import ctypes as C
import io
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRID = """
options: {{silent: True}}
grid: {{Lx: 1.e-2, Ly: 1.e-2, Nx: {n}, Ny: {n}, xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P'], yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P']}}
geometry: {{type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.}}
numerics: {{CFL: 0.5, adaptive: 1, tol: 1e-12, dt: 1e-10, max_it: 100000000}}
properties: {{shear: 0.0794, bulk: 0., EOS: DH, P0: 101325., rho0: 877.7007, C1: 3.5e10, C2: 1.23}}
"""


def stats(v):
    return {'median': statistics.median(v), 'min': min(v), 'max': max(v), 'all': list(v)}


def build(n, steps):
    from gapflow_amd import Problem
    with contextlib.redirect_stdout(io.StringIO()):
        p = Problem.from_string(GRID.format(n=n))
        p._pre_run()
        if steps:
            p._advance(steps, honor_stop=False)
    return p


def timed(dst, src, mode, reps):
    from gapflow_amd import _lib
    ms = C.c_double(0.)
    _lib.check(dst._lib.gpf_resample_time(dst._h, src._h, mode, reps, C.byref(ms)))
    return ms.value


def main(argv=None):
    cli = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    cli.add_argument('--src', type=int, default=1024)
    cli.add_argument('--dst', type=int, default=4096)
    cli.add_argument('--reps', type=int, default=20)
    cli.add_argument('--rounds', type=int, default=5)
    cli.add_argument('--json', metavar='FILE')
    o = cli.parse_args(argv)
    src, dst = build(o.src, 4), build(o.dst, 0)
    t = {'resample': [], 'store only': []}
    for r in range(o.rounds + 1):
        for mode, k in enumerate(t):
            v = timed(dst, src, mode, o.reps)
            if r:
                t[k].append(v)
    dst.init_from(src)          # the call itself, once, as a user makes it
    stored = 3 * o.dst * o.dst * 8
    out = {'library': os.environ.get('GPF_LIB_PATH', 'default'), 'src': o.src, 'dst': o.dst, 'reps': o.reps, 'rounds': o.rounds,
           'bytes_stored': stored, 'ms_per_call': {k: stats(v) for k, v in t.items()}}
    for k, v in out['ms_per_call'].items():
        print(f"{k:11s} {o.src}^2 -> {o.dst}^2: {v['median']:.4f} ms ({v['min']:.4f} .. {v['max']:.4f}), "
              f"{stored / v['median'] / 1e9:.2f} TB/s of stores")
    print(f"resample / store only: {out['ms_per_call']['resample']['median'] / out['ms_per_call']['store only']['median']:.2f}")
    if o.json:
        os.makedirs(os.path.dirname(os.path.abspath(o.json)), exist_ok=True)
        with open(o.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
