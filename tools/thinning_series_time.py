"""Cost of the shear-thinning series: ms per stage-wise step with nothing armed and with the series behind every step and behind
every tenth.

    python tools/thinning_series_time.py [--size 1024] [--steps 20] [--rounds 5] [--json FILE]

One process, one handle, alternating legs, one warm-up round that is thrown away, then --rounds rounds; every figure is printed
with its median and its whole range.  The case: a --size x --size Eyring problem on a 2-D gap (an asperity, periodic in both
directions).  A thinning problem steps stage-wise, the host between the calls, so every figure is the host's time for a step too.
Legs, all through gpf_thinning_series_time:
    unarmed     mode 0: the steps with the armed series put aside for the call
    every1      mode 1 with the series armed at every = 1
    every10     mode 1 with the series armed at every = 10
    added = (the leg - unarmed) per step; per RECORD that is ten times as much for every10
GPF_LIB_PATH selects another build of the library."""
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

CASE = """
options: {{silent: True}}
grid: {{Lx: 0.02, Ly: 0.02, Nx: {n}, Ny: {n}, xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P'], yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P']}}
geometry: {{type: asperity, hmin: 2.e-6, hmax: 1.e-5, num: 1, U: 0.5, V: 0.05}}
numerics: {{adaptive: 1, CFL: 0.4, tol: 1e-14, max_it: 100000000}}
properties:
    EOS: DH
    shear: 0.05
    bulk: 0.
    rho0: 877.7007
    thinning: {{name: Eyring, tauE: 5.e5}}
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


def timed(p, n, mode, every):
    from gapflow_amd import _lib
    p.set_thinning_series(every)
    ms = C.c_double(0.)
    _lib.check(p._lib.gpf_thinning_series_time(p._h, n, mode, C.byref(ms)))
    p._mark_device_advanced()
    return ms.value / n


def measure(p, steps, rounds):
    legs = [('unarmed', lambda: timed(p, steps, 0, 1)), ('every1', lambda: timed(p, steps, 1, 1)), ('every10', lambda: timed(p, steps, 1, 10))]
    t = {k: [] for k, _ in legs}
    for r in range(rounds + 1):
        for k, leg in legs:
            v = leg()
            if r:
                t[k].append(v)
    res = {'ms_per_step': {k: stats(v) for k, v in t.items()}}
    for k in ('every1', 'every10'):
        res[f'added_ms_per_step_{k}'] = stats([a - b for a, b in zip(t[k], t['unarmed'])])
    return res


def show(name, res):
    line = name
    for k, s in res['ms_per_step'].items():
        line += f"   {k} {s['median']:.4f} ms/step ({s['min']:.4f} .. {s['max']:.4f})"
    for k in ('every1', 'every10'):
        d = res[f'added_ms_per_step_{k}']
        line += f"   {k} added {d['median']:.4f} ({d['min']:.4f} .. {d['max']:.4f})"
    print(line)


def main(argv=None):
    cli = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    cli.add_argument('--size', type=int, default=1024)
    cli.add_argument('--steps', type=int, default=20)
    cli.add_argument('--rounds', type=int, default=5)
    cli.add_argument('--json', metavar='FILE')
    o = cli.parse_args(argv)
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
