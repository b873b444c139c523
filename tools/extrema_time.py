"""Cost of field extrema: ms per step without them and with a record behind every step.

    python tools/extrema_time.py [--small-steps 2000] [--size 4096] [--steps 100] [--rounds 5] [--unarmed-only] [--json FILE]

One process, alternating legs, one warm-up round that is thrown away, then --rounds rounds; every figure is printed with its
median and its whole range.  Two cases:
    small   the Nx = 100 1-D journal bearing (k_small_steps: the records are written inside the batch, which is not cut)
    large   a --size x --size journal bearing (k_step2: k_extrema_partial + k_extrema_fold behind every step), with
            gpf_stream_probe reading 4 planes of the same number of doubles and writing 1 beside it (it cannot write none:
            the yardstick moves 5/4 of the extrema's bytes, which the ratio is corrected for)
Legs:
    unarmed  gpf_extrema_time mode 0: the steps alone (armed extrema are put aside for the call)
    armed    gpf_extrema_time mode 1, every = 1
    added = armed - unarmed per step (HIP events on the handle's stream)
GPF_LIB_PATH selects another build of the library.  --unarmed-only times a build without gpf_extrema_* (the parent commit's):
the entries are dropped from the ctypes table before it loads, and the steps are timed with gpf_probes_time mode 0, which
enqueues the same launches: its `unarmed` is the figure to hold this build's against."""
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

SMALL = """
options: {silent: True}
grid: {dx: 1.e-5, dy: 1., Nx: 100, Ny: 1, xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P'], yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P']}
geometry: {type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.}
numerics: {CFL: 0.5, adaptive: 1, tol: 1e-12, dt: 1e-10, max_it: 100000000}
properties: {shear: 0.0794, bulk: 0., EOS: DH, P0: 101325., rho0: 877.7007, C1: 3.5e12, C2: 1.23}
"""
LARGE = """
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
        p._advance(4, honor_stop=False)
    return p


def timed(p, fn, n, mode):
    from gapflow_amd import _lib
    ms = C.c_double(0.)
    _lib.check(fn(p._h, n, mode, C.byref(ms)))
    return ms.value / n


def stream(lib, doubles):
    from gapflow_amd import _lib
    ms = C.c_double(0.)
    _lib.check(lib.gpf_stream_probe(0, 4, 1, doubles, 10, C.byref(ms)))
    return ms.value


def measure(p, steps, rounds, yard=None):
    from gapflow_amd import _lib
    has = 'gpf_extrema_time' in _lib.SIGNATURES
    legs = [('unarmed', lambda: timed(p, p._lib.gpf_extrema_time if has else p._lib.gpf_probes_time, steps, 0))]
    if has:
        p.set_extrema(1)
        legs.append(('armed', lambda: timed(p, p._lib.gpf_extrema_time, steps, 1)))
    if yard is not None:
        legs.append(('stream', yard))
    t = {k: [] for k, _ in legs}
    for r in range(rounds + 1):
        for k, leg in legs:
            v = leg()
            if r:
                t[k].append(v)
    res = {'ms_per_step': {k: stats(t[k]) for k in t if k != 'stream'}}
    if has:
        res['added_ms_per_record'] = stats([a - b for a, b in zip(t['armed'], t['unarmed'])])
    if yard is not None:
        res['stream_4in_1out_ms'] = stats(t['stream'])
        if has:
            res['ratio_added_to_stream_of_same_bytes'] = res['added_ms_per_record']['median'] / (statistics.median(t['stream']) * 4. / 5.)
    return res


def show(name, res):
    u = res['ms_per_step']['unarmed']
    line = f"{name:12s} unarmed {u['median']:.5f} ms/step ({u['min']:.5f} .. {u['max']:.5f})"
    if 'armed' in res['ms_per_step']:
        a, d = res['ms_per_step']['armed'], res['added_ms_per_record']
        line += f"   armed, every = 1 {a['median']:.5f} ({a['min']:.5f} .. {a['max']:.5f})   added {d['median']:.5f} ({d['min']:.5f} .. {d['max']:.5f})"
    if 'stream_4in_1out_ms' in res:
        line += f"   stream 4 in / 1 out {res['stream_4in_1out_ms']['median']:.4f}"
    if 'ratio_added_to_stream_of_same_bytes' in res:
        line += f"   added / stream of the same bytes {res['ratio_added_to_stream_of_same_bytes']:.2f}"
    print(line)


def main(argv=None):
    cli = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    cli.add_argument('--small-steps', type=int, default=2000)
    cli.add_argument('--size', type=int, default=4096)
    cli.add_argument('--steps', type=int, default=100)
    cli.add_argument('--rounds', type=int, default=5)
    cli.add_argument('--unarmed-only', action='store_true')
    cli.add_argument('--json', metavar='FILE')
    o = cli.parse_args(argv)
    if o.unarmed_only:
        from gapflow_amd import _lib
        for name in [k for k in _lib.SIGNATURES if k.startswith('gpf_extrema_')]:
            del _lib.SIGNATURES[name]
    out = {'library': os.environ.get('GPF_LIB_PATH', 'default'), 'rounds': o.rounds, 'cases': {}}
    p = build(SMALL)
    out['cases']['small Nx=100'] = dict(measure(p, o.small_steps, o.rounds), steps=o.small_steps)
    show('Nx = 100', out['cases']['small Nx=100'])
    del p
    if o.size > 0:
        n = o.size
        p = build(LARGE.format(n=n))
        out['cases'][f'{n}^2'] = dict(measure(p, o.steps, o.rounds, yard=lambda: stream(p._lib, (n + 2) * (n + 2))), steps=o.steps)
        show(f'{n}^2', out['cases'][f'{n}^2'])
    if o.json:
        os.makedirs(os.path.dirname(os.path.abspath(o.json)), exist_ok=True)
        with open(o.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
