"""Cost of the region series: what a record behind every step adds for K = 1 and K = 8 regions, next to the weighted film
integrals' record at the same K in the same process, and to the step with nothing armed.

    python tools/regions_time.py [--sizes 4096] [--steps 50] [--rounds 5] [--json FILE]

One process, alternating legs, one warm-up round that is thrown away, then --rounds rounds; every figure is printed with its
median and its whole range.  Per size n, for an x-only gap (journal bearing) and a 2-D gap (asperity):
    off         gpf_regions_time mode 0: the steps alone, nothing armed
    weighted K  gpf_weighted_time mode 1, every = 1, K smooth planes: k_wfilm_partial (grid Nx x K) + k_wfilm_fold behind every step
    regions K   gpf_regions_time mode 1, every = 1, K regions: k_region_partial (grid Nx x K) + k_region_fold behind every step
    added = leg - off per recorded step (HIP events on the handle's stream); ratio = added(regions K) / added(weighted K);
    spread = max - min of added(weighted K) over the rounds: what the difference between the two is to be held against.
The regions are bands between quantiles of the state's own rho, h and jx after the warm-up steps; the share of the film each holds
goes into the JSON (cells_share).  Membership does not change the work: every cell is added with a weight of 1.0 or 0.0.  The
expectation: a region record reads one plane fewer per cell
than a weighted record and evaluates one predicate more, so it should cost no more."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402

from tools.integrals_time import GAPS, TEXT, stats      # noqa: E402  (the integrals' inputs: the same problems)
from tools.weighted_time import build, planes, timed   # noqa: E402


def regions(p, K):
    q, h = np.array(p.q)[:, 1:-1, 1:-1], np.array(p.topo.full[0])[1:-1, 1:-1]
    fields = (('rho', q[0]), ('h', h), ('jx', q[1]))
    out = []
    for k in range(K):
        name, f = fields[k % 3]
        lo, hi = float(np.quantile(f, 0.1 + 0.1 * (k // 3))), float(np.quantile(f, 0.9 - 0.1 * (k // 3)))
        out.append({'field': name, 'above': lo, 'below': hi if hi > lo else float('inf')})
    return out


def main(argv=None):
    cli = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    cli.add_argument('--sizes', type=int, nargs='+', default=[4096])
    cli.add_argument('--steps', type=int, default=50)
    cli.add_argument('--rounds', type=int, default=5)
    cli.add_argument('--regions', type=int, nargs='+', default=[1, 8])
    cli.add_argument('--json', metavar='FILE')
    o = cli.parse_args(argv)
    out = {'steps': o.steps, 'rounds': o.rounds, 'cases': {}}
    for n in o.sizes:
        for gap, geo in GAPS.items():
            p = build(TEXT.format(n=n, geo=geo))
            res = {}
            for K in o.regions:
                p.set_weighted_integrals(planes(p.grid, K))
                p.set_regions(regions(p, K))
                t = {'off': [], 'weighted': [], 'regions': []}
                for r in range(o.rounds + 1):
                    legs = (('off', lambda: timed(p, 'gpf_regions_time', o.steps, 0)), ('weighted', lambda: timed(p, 'gpf_weighted_time', o.steps, 1)),
                            ('regions', lambda: timed(p, 'gpf_regions_time', o.steps, 1)))
                    for k, leg in legs:
                        v = leg()
                        if r:
                            t[k].append(v)
                add_w = [a - b for a, b in zip(t['weighted'], t['off'])]
                add_r = [a - b for a, b in zip(t['regions'], t['off'])]
                a = res[f'K={K}'] = {'ms_per_step': {k: stats(t[k]) for k in t}, 'added_ms_per_record_weighted': stats(add_w),
                                     'added_ms_per_record_regions': stats(add_r), 'spread_weighted_ms': max(add_w) - min(add_w),
                                     'ratio_regions_to_weighted': statistics.median(add_r) / statistics.median(add_w),
                                     'cells_share': (p.film_regions()['cells'] / (n * n)).tolist()}
                print(f"{n}^2 {gap:7s} K = {K}: off {a['ms_per_step']['off']['median']:.4f} ms/step   weighted added "
                      f"{a['added_ms_per_record_weighted']['median']:.4f} ({a['added_ms_per_record_weighted']['min']:.4f} .. "
                      f"{a['added_ms_per_record_weighted']['max']:.4f})   regions added {a['added_ms_per_record_regions']['median']:.4f} "
                      f"({a['added_ms_per_record_regions']['min']:.4f} .. {a['added_ms_per_record_regions']['max']:.4f})   regions / weighted "
                      f"{a['ratio_regions_to_weighted']:.2f}   spread of the weighted leg {a['spread_weighted_ms']:.4f}", flush=True)
            out['cases'][f'{n}^2 {gap}'] = res
            del p
    if o.json:
        os.makedirs(os.path.dirname(os.path.abspath(o.json)), exist_ok=True)
        with open(o.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
