"""Cost of weighted film integrals: what a record behind every step adds for K = 1 and K = 8 weight planes, next to the film
integrals' record and to the step with nothing armed.

    python tools/weighted_time.py [--sizes 4096] [--steps 50] [--rounds 5] [--json FILE]

One process, alternating legs, one warm-up round that is thrown away, then --rounds rounds; every figure is printed with its
median and its whole range.  Per size n, for an x-only gap (journal bearing) and a 2-D gap (asperity):
    off         gpf_weighted_time mode 0: the steps alone, nothing armed
    integrals   gpf_integrals_time mode 1, every = 1: k_film_partial + k_film_fold behind every step
    weighted K  gpf_weighted_time mode 1, every = 1, K smooth planes: k_wfilm_partial (grid Nx x K) + k_wfilm_fold behind every step
    added = leg - off per recorded step (HIP events on the handle's stream); ratio = added(weighted K) / added(integrals).
The expectation to hold the figures against: K closure passes whose q / topo reads are mostly served from the L2 behind the first
weight's workgroup, plus one read of each weight plane -- about K times the integrals' record, or less."""
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

from tools.integrals_time import GAPS, TEXT, stats      # noqa: E402  (the integrals' inputs: the same problems)


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
    _lib.check(getattr(p._lib, fn)(p._h, n, mode, C.byref(ms)))
    return ms.value / n


def planes(grid, K):
    from gapflow_amd import weights
    return [weights.mode(grid, k // 2 + 1, k % 3, 'cos' if k % 2 else 'sin') for k in range(K)]


def main(argv=None):
    cli = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    cli.add_argument('--sizes', type=int, nargs='+', default=[4096])
    cli.add_argument('--steps', type=int, default=50)
    cli.add_argument('--rounds', type=int, default=5)
    cli.add_argument('--planes', type=int, nargs='+', default=[1, 8])
    cli.add_argument('--json', metavar='FILE')
    o = cli.parse_args(argv)
    out = {'steps': o.steps, 'rounds': o.rounds, 'cases': {}}
    for n in o.sizes:
        for gap, geo in GAPS.items():
            p = build(TEXT.format(n=n, geo=geo))
            p.set_integrals(1)
            res = {}
            for K in o.planes:
                p.set_weighted_integrals(planes(p.grid, K))
                t = {'off': [], 'integrals': [], 'weighted': []}
                for r in range(o.rounds + 1):
                    legs = (('off', lambda: timed(p, 'gpf_weighted_time', o.steps, 0)), ('integrals', lambda: timed(p, 'gpf_integrals_time', o.steps, 1)),
                            ('weighted', lambda: timed(p, 'gpf_weighted_time', o.steps, 1)))
                    for k, leg in legs:
                        v = leg()
                        if r:
                            t[k].append(v)
                add_i = [a - b for a, b in zip(t['integrals'], t['off'])]
                add_w = [a - b for a, b in zip(t['weighted'], t['off'])]
                res[f'K={K}'] = {'ms_per_step': {k: stats(t[k]) for k in t}, 'added_ms_per_record_integrals': stats(add_i),
                                 'added_ms_per_record_weighted': stats(add_w),
                                 'ratio_weighted_to_integrals': statistics.median(add_w) / statistics.median(add_i)}
                a = res[f'K={K}']
                print(f"{n}^2 {gap:7s} K = {K}: off {a['ms_per_step']['off']['median']:.4f} ms/step   integrals added "
                      f"{a['added_ms_per_record_integrals']['median']:.4f} ({a['added_ms_per_record_integrals']['min']:.4f} .. "
                      f"{a['added_ms_per_record_integrals']['max']:.4f})   weighted added {a['added_ms_per_record_weighted']['median']:.4f} "
                      f"({a['added_ms_per_record_weighted']['min']:.4f} .. {a['added_ms_per_record_weighted']['max']:.4f})   weighted / integrals "
                      f"{a['ratio_weighted_to_integrals']:.2f}", flush=True)
            out['cases'][f'{n}^2 {gap}'] = res
            del p
    if o.json:
        os.makedirs(os.path.dirname(os.path.abspath(o.json)), exist_ok=True)
        with open(o.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
