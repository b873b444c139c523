"""Cost of film integrals: what a record behind every step adds, against a read-only stream of the same bytes.

    python tools/integrals_time.py [--sizes 1024 4096] [--steps 100] [--rounds 5] [--json FILE]

One process, alternating legs, one warm-up round that is thrown away, then --rounds rounds; every figure is printed with its
median and its whole range.  Per size n, for an x-only gap (journal bearing: k_step2 reads the row-coefficient table, the
integrals read the gap planes all the same) and a 2-D gap (asperity):
    off        gpf_integrals_time mode 0: the steps alone
    integrals  gpf_integrals_time mode 1, every = 1: k_film_partial + k_film_fold behind every step
    added = integrals - off per recorded step (HIP events on the handle's stream)
    stream     gpf_stream_probe reading 6 planes of the same number of doubles and writing 1 (it cannot write none: one plane out
               makes the yardstick 7/6 of the integrals' bytes, which the ratio below is corrected for)
    ratio = added / (stream * 6 / 7); the scaling takes a byte written to cost what a byte read costs, so the unscaled stream
    time and added / stream are printed beside it"""
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

TEXT = """
options: {{silent: True}}
grid: {{dx: 1.e-5, dy: 1.e-5, Nx: {n}, Ny: {n}, xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P'], yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P']}}
geometry: {geo}
numerics: {{CFL: 0.5, adaptive: 1, tol: 1e-12, dt: 1e-10, max_it: 100000000}}
properties: {{shear: 0.0794, bulk: 0., EOS: DH, P0: 101325., rho0: 877.7007, C1: 3.5e10, C2: 1.23}}
"""
GAPS = {'x-only': "{type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.}",
        '2-d': "{type: asperity, hmin: 2.e-6, hmax: 1.e-5, num: 1, U: 0.1, V: 0.05}"}


def stats(v):
    return {'median': statistics.median(v), 'min': min(v), 'max': max(v), 'all': list(v)}


def build(text):
    from gapflow_amd import Problem
    with contextlib.redirect_stdout(io.StringIO()):
        p = Problem.from_string(text)
        p._pre_run()
        p._advance(4, honor_stop=False)
    return p


def timed(p, n, mode):
    from gapflow_amd import _lib
    ms = C.c_double(0.)
    _lib.check(p._lib.gpf_integrals_time(p._h, n, mode, C.byref(ms)))
    return ms.value / n


def stream(lib, doubles):
    from gapflow_amd import _lib
    ms = C.c_double(0.)
    _lib.check(lib.gpf_stream_probe(0, 6, 1, doubles, 10, C.byref(ms)))
    return ms.value


def main(argv=None):
    cli = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    cli.add_argument('--sizes', type=int, nargs='+', default=[1024, 4096])
    cli.add_argument('--steps', type=int, default=100)
    cli.add_argument('--rounds', type=int, default=5)
    cli.add_argument('--json', metavar='FILE')
    o = cli.parse_args(argv)
    out = {'steps': o.steps, 'rounds': o.rounds, 'cases': {}}
    for n in o.sizes:
        for gap, geo in GAPS.items():
            p = build(TEXT.format(n=n, geo=geo))
            p.set_integrals(1)
            t = {'off': [], 'integrals': [], 'stream': []}
            for r in range(o.rounds + 1):
                legs = (('off', lambda: timed(p, o.steps, 0)), ('integrals', lambda: timed(p, o.steps, 1)),
                        ('stream', lambda: stream(p._lib, (n + 2) * (n + 2))))
                for k, leg in legs:
                    v = leg()
                    if r:
                        t[k].append(v)
            added = [a - b for a, b in zip(t['integrals'], t['off'])]
            yard = [s * 6. / 7. for s in t['stream']]
            res = {'ms_per_step': {k: stats(t[k]) for k in ('off', 'integrals')}, 'stream_6in_1out_ms': stats(t['stream']),
                   'added_ms_per_record': stats(added), 'ratio_added_to_stream_of_same_bytes': statistics.median(added) / statistics.median(yard),
                   'ratio_added_to_stream_unscaled': statistics.median(added) / statistics.median(t['stream'])}
            out['cases'][f'{n}^2 {gap}'] = res
            print(f"{n}^2 {gap:7s} off {res['ms_per_step']['off']['median']:.4f} ms/step   with integrals {res['ms_per_step']['integrals']['median']:.4f}"
                  f"   added {res['added_ms_per_record']['median']:.4f} ({res['added_ms_per_record']['min']:.4f} .. {res['added_ms_per_record']['max']:.4f})"
                  f"   stream 6 in / 1 out {res['stream_6in_1out_ms']['median']:.4f}   added / stream of the same bytes {res['ratio_added_to_stream_of_same_bytes']:.2f}"
                  f" (unscaled {res['ratio_added_to_stream_unscaled']:.2f})")
            del p
    if o.json:
        os.makedirs(os.path.dirname(os.path.abspath(o.json)), exist_ok=True)
        with open(o.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
