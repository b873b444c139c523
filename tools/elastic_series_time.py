"""Cost of an elastic problem's series: ms per step with nothing armed, with film integrals and with the deformation series behind
every step.

    python tools/elastic_series_time.py [--size 1024] [--steps 20] [--rounds 5] [--unarmed-only] [--json FILE]

One process, alternating legs, one warm-up round that is thrown away, then --rounds rounds; every figure is printed with its
median and its whole range.  The case: a --size x --size parabolic slider with an elastic gap, periodic in both directions
(tests/test_gpu_elastic.py's 'periodic_2d' on a larger grid).  An elastic problem steps stage-wise, the host between the calls,
so every figure is the host's time for a step too.  Legs:
    update      time.perf_counter around --steps Problem.update() calls with nothing armed (ends in the calls' own synchronises)
    unarmed     gpf_elastic_series_time mode 0: the same steps inside the library (armed series are put aside for the call)
    integrals   gpf_integrals_time mode 1, film integrals at every = 1
    series      gpf_elastic_series_time mode 1, the deformation series at every = 1
    added = the leg - unarmed, per step
GPF_LIB_PATH selects another build of the library.  --unarmed-only times a build without gpf_elastic_series_* (the parent
commit's): the entries are dropped from the ctypes table before it loads and only the `update` leg runs: it is the figure to
hold this build's `update` against."""
import argparse
import contextlib
import ctypes as C
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASE = """
options: {{silent: True}}
grid: {{Lx: 0.0762, Ly: 0.04, Nx: {n}, Ny: {n}}}
geometry: {{type: parabolic, hmin: 2.54e-5, hmax: 5.08e-5, U: 4.57, V: 0.3}}
numerics: {{adaptive: 1, CFL: 0.45, tol: 1e-12, dt: 1.e-10, max_it: 100000000}}
properties:
    EOS: Bayada
    rho0: 850.
    shear: 0.039
    bulk: 0.
    cl: 1600.
    cv: 352.
    elastic: {{E: 50e09, v: 0.3, alpha_underrelax: 0.05}}
    piezo: {{name: Dukler, shearv: 3.9e-5, rhol: 850., rhov: 0.019}}
"""


def stats(v):
    return {'median': statistics.median(v), 'min': min(v), 'max': max(v), 'all': list(v)}


def build(text):
    from gapflow_amd import Problem
    with contextlib.redirect_stdout(io.StringIO()):
        p = Problem.from_string(text)
        p._pre_run()
        for _ in range(3):
            p.update()
    return p


def timed(p, fn, n, mode):
    from gapflow_amd import _lib
    ms = C.c_double(0.)
    _lib.check(fn(p._h, n, mode, C.byref(ms)))
    p._mark_device_advanced()
    return ms.value / n


def updates(p, n):
    t0 = time.perf_counter()
    for _ in range(n):
        p.update()
    return (time.perf_counter() - t0) * 1e3 / n


def measure(p, steps, rounds):
    from gapflow_amd import _lib
    has = 'gpf_elastic_series_time' in _lib.SIGNATURES
    legs = [('update', lambda: updates(p, steps))]
    if has:
        p.set_integrals(1)
        p.set_elastic_series(1)
        legs[0] = ('update', lambda: (p.clear_integrals(), p.clear_elastic_series(), updates(p, steps), p.set_integrals(1), p.set_elastic_series(1))[2])
        legs += [('unarmed', lambda: timed(p, p._lib.gpf_elastic_series_time, steps, 0)),
                 ('integrals', lambda: timed(p, p._lib.gpf_integrals_time, steps, 1)),
                 ('series', lambda: timed(p, p._lib.gpf_elastic_series_time, steps, 1))]
    t = {k: [] for k, _ in legs}
    for r in range(rounds + 1):
        for k, leg in legs:
            v = leg()
            if r:
                t[k].append(v)
    res = {'ms_per_step': {k: stats(v) for k, v in t.items()}}
    if has:
        for k in ('integrals', 'series'):
            res[f'added_ms_per_record_{k}'] = stats([a - b for a, b in zip(t[k], t['unarmed'])])
    return res


def show(name, res):
    line = name
    for k, s in res['ms_per_step'].items():
        line += f"   {k} {s['median']:.4f} ms/step ({s['min']:.4f} .. {s['max']:.4f})"
    for k in ('integrals', 'series'):
        d = res.get(f'added_ms_per_record_{k}')
        if d:
            line += f"   {k} added {d['median']:.4f} ({d['min']:.4f} .. {d['max']:.4f})"
    print(line)


def main(argv=None):
    cli = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    cli.add_argument('--size', type=int, default=1024)
    cli.add_argument('--steps', type=int, default=20)
    cli.add_argument('--rounds', type=int, default=5)
    cli.add_argument('--unarmed-only', action='store_true')
    cli.add_argument('--json', metavar='FILE')
    o = cli.parse_args(argv)
    if o.unarmed_only:
        from gapflow_amd import _lib
        for name in [k for k in _lib.SIGNATURES if k.startswith('gpf_elastic_series_')]:
            del _lib.SIGNATURES[name]
    n = o.size
    p = build(CASE.format(n=n))
    out = {'library': os.environ.get('GPF_LIB_PATH', 'default'), 'rounds': o.rounds, 'steps': o.steps, 'cases': {f'{n}^2': measure(p, o.steps, o.rounds)}}
    show(f'{n}^2', out['cases'][f'{n}^2'])
    if o.json:
        os.makedirs(os.path.dirname(os.path.abspath(o.json)), exist_ok=True)
        with open(o.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
