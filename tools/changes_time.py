"""Cost of the step-change series: ms per step with nothing armed and with a record behind every step.

    python tools/changes_time.py [--size 4096] [--steps 20] [--rounds 5] [--planes] [--unarmed-only] [--json FILE] [--label TEXT]

One process, alternating legs, one warm-up round that is thrown away, then --rounds rounds; every figure is printed with its
median and its whole range.  The case: bench.py's flagship workload, a --size x --size journal bearing periodic in both
directions (an x-only gap: the step moves 48 B per cell), and with --planes the same grid with a 2-D gap (72 B per cell).  Legs:
    unarmed     gpf_changes_time mode 0: the steps as gpf_step enqueues them, armed series put aside for the call
    changes     gpf_changes_time mode 1, the series at every = 1: k_change_partial + k_change_fold behind every step
    added = changes - unarmed, per record (the record reads 56 B per cell)
GPF_LIB_PATH selects another build of the library.  --unarmed-only times a build without gpf_changes_* (the parent commit's):
the entries are dropped from the ctypes table before it loads and the `unarmed` leg goes through gpf_extrema_time mode 0, which
enqueues the same steps: it is the figure to hold this build's `unarmed` against."""
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
grid: {{dx: 1.e-5, dy: 1.e-5, Nx: {n}, Ny: {n}, xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P'], yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P']}}
geometry: {{type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.}}
numerics: {{CFL: 0.5, adaptive: 1, tol: 1e-12, dt: 1e-10, max_it: 100000000}}
properties: {{shear: 0.0794, bulk: 0., EOS: DH, P0: 101325., rho0: 877.7007, C1: 3.5e10, C2: 1.23}}
"""


def stats(v):
    return {'median': statistics.median(v), 'min': min(v), 'max': max(v), 'all': list(v)}


def build(text):
    from gapflow_amd import Problem
    with contextlib.redirect_stdout(io.StringIO()):
        p = Problem.from_string(text)
        p._pre_run()
        p._advance(4, honor_stop=False)         # the step plan's trial launches happen here
    return p


def timed(p, fn, n, mode):
    from gapflow_amd import _lib
    ms = C.c_double(0.)
    _lib.check(fn(p._h, n, mode, C.byref(ms)))
    p._mark_device_advanced()
    return ms.value / n


def measure(p, steps, rounds):
    from gapflow_amd import _lib
    has = 'gpf_changes_time' in _lib.SIGNATURES
    if has:
        p.set_changes(1)
        legs = [('unarmed', lambda: timed(p, p._lib.gpf_changes_time, steps, 0)),
                ('changes', lambda: timed(p, p._lib.gpf_changes_time, steps, 1))]
    else:
        legs = [('unarmed', lambda: timed(p, p._lib.gpf_extrema_time, steps, 0))]
    t = {k: [] for k, _ in legs}
    for r in range(rounds + 1):
        for k, leg in legs:
            v = leg()
            if r:
                t[k].append(v)
    res = {'ms_per_step': {k: stats(v) for k, v in t.items()}}
    if has:
        res['added_ms_per_record'] = stats([a - b for a, b in zip(t['changes'], t['unarmed'])])
    return res


def show(name, res):
    line = name
    for k, s in res['ms_per_step'].items():
        line += f"   {k} {s['median']:.4f} ms/step ({s['min']:.4f} .. {s['max']:.4f})"
    d = res.get('added_ms_per_record')
    if d:
        line += f"   added {d['median']:.4f} ms/record ({d['min']:.4f} .. {d['max']:.4f})"
    print(line)


def main(argv=None):
    cli = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    cli.add_argument('--size', type=int, default=4096)
    cli.add_argument('--steps', type=int, default=20)
    cli.add_argument('--rounds', type=int, default=5)
    cli.add_argument('--planes', action='store_true', help='also the same grid with the gap read from planes (GPF_TOPO_PLANES)')
    cli.add_argument('--unarmed-only', action='store_true')
    cli.add_argument('--json', metavar='FILE')
    cli.add_argument('--label', help="what the JSON names as its library (default: GPF_LIB_PATH's value, or 'default')")
    o = cli.parse_args(argv)
    if o.unarmed_only:
        from gapflow_amd import _lib
        for name in [k for k in _lib.SIGNATURES if k.startswith('gpf_changes_')]:
            del _lib.SIGNATURES[name]
    n = o.size
    out = {'library': o.label or os.environ.get('GPF_LIB_PATH', 'default'), 'rounds': o.rounds, 'steps': o.steps, 'cases': {}}
    for label, planes in [(f'{n}^2 x-only gap', False)] + ([(f'{n}^2 gap planes', True)] if o.planes else []):
        if planes:
            os.environ['GPF_TOPO_PLANES'] = '1'
        p = build(CASE.format(n=n))
        out['cases'][label] = measure(p, o.steps, o.rounds)
        show(label, out['cases'][label])
        del p
    if o.json:
        os.makedirs(os.path.dirname(os.path.abspath(o.json)), exist_ok=True)
        with open(o.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
