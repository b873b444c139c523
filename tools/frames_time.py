"""Cost of the reduced frames: what a block-mean record behind every step adds, next to the film integrals' record -- which reads the
same planes once and evaluates the same closures -- in the same process and to the step with nothing armed; and what a picture of
the film costs from launch to the host array, next to a written frame (`write()`), the only way to a 2-D field before.

    python tools/frames_time.py [--sizes 4096] [--steps 20] [--rounds 5] [--stride 8 8] [--write-rounds 2] [--gaps x-only] [--json FILE]

One process, alternating legs, one warm-up round that is thrown away, then --rounds rounds; every figure is printed with its
median and its whole range.  Per size n and gap:
    off          gpf_frames_time mode 0: the steps alone, nothing armed
    integrals    gpf_integrals_time mode 1, every = 1: k_film_partial (grid Nx) + k_film_fold behind every step
    mean-9       gpf_frames_time mode 1, every = 1: all nine fields, mean over --stride blocks, f4 (k_frame_mean<.., NEED_TAU>)
    mean-4       ... rho, jx, jy, p (24 B per window cell; TB/s = 24 n^2 / added time)
    sample-4     ... rho, jx, jy, p sampled at the blocks' first cells (k_frame_sample)
    added = leg - off per recorded step (HIP events on the handle's stream); spread = max - min of added(integrals) over the
    rounds: what a difference between mean-9 and the integrals is to be held against.
    frame_now    wall time of Problem.frame_now(stride, reduce='mean') of rho, jx, jy, p: launch, copy, split into arrays
    write        wall time of write(scalars=False, fields=True, params=False) on a problem that is not silent (--write-rounds
                 after one warm-up; 0: skipped -- every written frame adds 28 planes to sol.nc in a temporary directory, which
                 is removed)"""
import argparse
import contextlib
import io
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.integrals_time import GAPS, TEXT, stats      # noqa: E402  (the integrals' inputs: the same problems)
from tools.weighted_time import build, timed           # noqa: E402

ALL = ('rho', 'jx', 'jy', 'p', 'h', 'tau_xz_bot', 'tau_yz_bot', 'tau_xz_top', 'tau_yz_top')


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main(argv=None):
    cli = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    cli.add_argument('--sizes', type=int, nargs='+', default=[4096])
    cli.add_argument('--steps', type=int, default=20)
    cli.add_argument('--rounds', type=int, default=5)
    cli.add_argument('--stride', type=int, nargs=2, default=[8, 8])
    cli.add_argument('--write-rounds', type=int, default=2)
    cli.add_argument('--gaps', nargs='+', default=['x-only'], choices=list(GAPS))
    cli.add_argument('--json', metavar='FILE')
    o = cli.parse_args(argv)
    stride = tuple(o.stride)
    out = {'steps': o.steps, 'rounds': o.rounds, 'stride': stride, 'cases': {}}
    for n in o.sizes:
        frames = {'mean-9': dict(fields=ALL, reduce='mean'), 'mean-4': dict(reduce='mean'), 'sample-4': dict(reduce='sample')}
        for gap in o.gaps:
            p = build(TEXT.format(n=n, geo=GAPS[gap]))
            p.set_integrals(1)
            t = {k: [] for k in ('off', 'integrals') + tuple(frames) + ('frame_now',)}

            def frame_leg(spec):
                p.set_frames(1, stride=stride, capacity=o.steps, **spec)
                return timed(p, 'gpf_frames_time', o.steps, 1)
            for r in range(o.rounds + 1):
                legs = [('off', lambda: timed(p, 'gpf_frames_time', o.steps, 0)), ('integrals', lambda: timed(p, 'gpf_integrals_time', o.steps, 1))]
                legs += [(k, lambda s=s: frame_leg(s)) for k, s in frames.items()]
                legs += [('frame_now', lambda: wall(lambda: p.frame_now(stride=stride, reduce='mean')))]
                for k, leg in legs:
                    v = leg()
                    if r:
                        t[k].append(v)
            p.clear_frames()
            added = {k: [a - b for a, b in zip(t[k], t['off'])] for k in t if k not in ('off', 'frame_now')}
            mx, my = -(-n // stride[0]), -(-n // stride[1])
            res = out['cases'][f'{n}^2 {gap}'] = {
                'ms_per_step': {k: stats(v) for k, v in t.items() if k != 'frame_now'},
                'added_ms_per_record': {k: stats(v) for k, v in added.items()},
                'spread_integrals_ms': max(added['integrals']) - min(added['integrals']),
                'mean4_TB_per_s': stats([24.0 * n * n / (a * 1e-3) / 1e12 for a in added['mean-4']]),
                'frame_now_wall_ms': stats(t['frame_now']), 'frame_now_bytes_to_host': 4 * mx * my * 4}
            print(f"{n}^2 {gap:7s}: off {res['ms_per_step']['off']['median']:.4f} ms/step ({res['ms_per_step']['off']['min']:.4f} .. "
                  f"{res['ms_per_step']['off']['max']:.4f});  added ms per record: " +
                  ';  '.join(f"{k} {a['median']:.4f} ({a['min']:.4f} .. {a['max']:.4f})" for k, a in res['added_ms_per_record'].items()) +
                  f";  spread of the integrals leg {res['spread_integrals_ms']:.4f};  mean-4 {res['mean4_TB_per_s']['median']:.2f} TB/s "
                  f"({res['mean4_TB_per_s']['min']:.2f} .. {res['mean4_TB_per_s']['max']:.2f}) of 24 B per cell;  frame_now wall "
                  f"{res['frame_now_wall_ms']['median']:.3f} ms ({res['frame_now_wall_ms']['min']:.3f} .. {res['frame_now_wall_ms']['max']:.3f}), "
                  f"{res['frame_now_bytes_to_host']} bytes to the host", flush=True)
            del p
            if o.write_rounds > 0:
                tmp = tempfile.mkdtemp(prefix='frames_time_')
                try:
                    from gapflow_amd import Problem
                    text = TEXT.format(n=n, geo=GAPS[gap]).replace('silent: True', f'silent: False, output: {tmp}/run, use_tstamp: False, write_freq: 1000000')
                    with contextlib.redirect_stdout(io.StringIO()):
                        w = Problem.from_string(text)
                        w._pre_run()
                        w._advance(4, honor_stop=False)
                    ms = []
                    for r in range(o.write_rounds + 1):
                        with contextlib.redirect_stdout(io.StringIO()):
                            w._advance(1, honor_stop=False)         # a frame is written of a state that has just been stepped to
                            v = wall(lambda: w.write(scalars=False, fields=True, params=False))
                        if r:
                            ms.append(v)
                    res['write_wall_ms'] = stats(ms)
                    res['write_bytes_to_host'] = 28 * (n + 2) * (n + 2) * 8
                    print(f"{n}^2 {gap:7s}: write(fields) wall {res['write_wall_ms']['median']:.1f} ms ({res['write_wall_ms']['min']:.1f} .. "
                          f"{res['write_wall_ms']['max']:.1f}), {res['write_bytes_to_host']} bytes to the host", flush=True)
                    w._writer.close()
                    del w
                finally:
                    shutil.rmtree(tmp, ignore_errors=True)
    if o.json:
        os.makedirs(os.path.dirname(os.path.abspath(o.json)), exist_ok=True)
        with open(o.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
