"""Cost of the line profiles: what a record behind every step adds for one centre line and for a full-width band mean, along x and
along y, next to the film integrals' record -- which reads the same planes once -- in the same process, and to the step with
nothing armed.

    python tools/lines_time.py [--sizes 4096] [--steps 50] [--rounds 5] [--gaps x-only] [--json FILE]

One process, alternating legs, one warm-up round that is thrown away, then --rounds rounds; every figure is printed with its
median and its whole range.  Per size n and gap:
    off          gpf_lines_time mode 0: the steps alone, nothing armed
    integrals    gpf_integrals_time mode 1, every = 1: k_film_partial (grid Nx) + k_film_fold behind every step
    centre-x     gpf_lines_time mode 1, every = 1, [{along: x}]: k_line_point, n threads, each lane its own cache line per plane
    centre-y     ... [{along: y}]: k_line_point, n threads, contiguous loads
    band-x       ... [{along: x, at: (1, n)}]: k_line_band_x, one wave per row over the whole width
    band-y       ... [{along: y, at: (1, n)}]: k_line_band_y_partial (n / 32 chunks x n threads) + k_line_band_y_fold
    added = leg - off per recorded step (HIP events on the handle's stream); spread = max - min of added(integrals) over the
    rounds: what a difference between a band and the integrals is to be held against."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.integrals_time import GAPS, TEXT, stats      # noqa: E402  (the integrals' inputs: the same problems)
from tools.weighted_time import build, timed           # noqa: E402


def main(argv=None):
    cli = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    cli.add_argument('--sizes', type=int, nargs='+', default=[4096])
    cli.add_argument('--steps', type=int, default=50)
    cli.add_argument('--rounds', type=int, default=5)
    cli.add_argument('--gaps', nargs='+', default=['x-only'], choices=list(GAPS))
    cli.add_argument('--json', metavar='FILE')
    o = cli.parse_args(argv)
    out = {'steps': o.steps, 'rounds': o.rounds, 'cases': {}}
    for n in o.sizes:
        lines = {'centre-x': {'along': 'x'}, 'centre-y': {'along': 'y'}, 'band-x': {'along': 'x', 'at': (1, n)}, 'band-y': {'along': 'y', 'at': (1, n)}}
        for gap in o.gaps:
            p = build(TEXT.format(n=n, geo=GAPS[gap]))
            p.set_integrals(1)
            t = {k: [] for k in ('off', 'integrals') + tuple(lines)}

            def line_leg(entry):
                p.set_lines([entry], 1, o.steps)
                return timed(p, 'gpf_lines_time', o.steps, 1)
            for r in range(o.rounds + 1):
                legs = [('off', lambda: timed(p, 'gpf_lines_time', o.steps, 0)), ('integrals', lambda: timed(p, 'gpf_integrals_time', o.steps, 1))]
                legs += [(k, lambda e=e: line_leg(e)) for k, e in lines.items()]
                for k, leg in legs:
                    v = leg()
                    if r:
                        t[k].append(v)
            p.clear_lines()
            added = {k: [a - b for a, b in zip(t[k], t['off'])] for k in t if k != 'off'}
            res = out['cases'][f'{n}^2 {gap}'] = {'ms_per_step': {k: stats(v) for k, v in t.items()},
                                                  'added_ms_per_record': {k: stats(v) for k, v in added.items()},
                                                  'spread_integrals_ms': max(added['integrals']) - min(added['integrals'])}
            print(f"{n}^2 {gap:7s}: off {res['ms_per_step']['off']['median']:.4f} ms/step ({res['ms_per_step']['off']['min']:.4f} .. "
                  f"{res['ms_per_step']['off']['max']:.4f});  added ms per record: " +
                  ';  '.join(f"{k} {a['median']:.4f} ({a['min']:.4f} .. {a['max']:.4f})" for k, a in res['added_ms_per_record'].items()) +
                  f";  spread of the integrals leg {res['spread_integrals_ms']:.4f}", flush=True)
            del p
    if o.json:
        os.makedirs(os.path.dirname(os.path.abspath(o.json)), exist_ok=True)
        with open(o.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
