"""Cost of the running field statistics: what one record adds to a step, for one field and for all four, next to an elementwise
kernel that moves the same bytes in the same process.

    python tools/stats_time.py [--sizes 4096] [--steps 20] [--rounds 5] [--json FILE]
    python tools/stats_time.py --step-time 200 [--arm 100] [--sizes 4096]

One process, alternating legs, one warm-up round that is thrown away, then --rounds rounds; every figure is printed with its
median and its whole range.  Per size n, on a 2-D gap (asperity), for fields = (p) and (p, rho, jx, jy):
    off      gpf_stats_time mode 0: the steps alone, nothing armed
    record   gpf_stats_time mode 1, every = 1: k_stats_update behind every step
    stream   gpf_stats_time mode 2: k_stats_stream, the elementwise kernel that reads the q planes a record reads and reads and
             writes its accumulator planes, 16 bytes per lane and access, same grid and same cache hint, no arithmetic
    probe    gpf_stream_probe(5 planes in, 4 out) for one field (the library's own probe holds at most 8 planes each way, so the
             four-field record has no counterpart there)
    added = record - off per recorded step (HIP events on the handle's stream); fraction = stream / added, probe / added.
The expectation to hold the figures against: 64 bytes of accumulators per field and cell plus 8 per q plane read -- 1.2 GB for
one field and 4.7 GB for four at 4096^2 -- at what this device streams.

--step-time N: the time of a step as gpf_step takes it, N steps per call, three calls after a warm-up, by the host's clock around
calls that end in a synchronise; --arm S arms all four fields at stride S first, where the library has statistics.  One JSON
line; meant to be run in alternating processes against another checkout of the project."""
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

from tools.integrals_time import GAPS, TEXT, stats      # noqa: E402  (the integrals' inputs: the same problems)


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
    _lib.check(p._lib.gpf_stats_time(p._h, n, mode, C.byref(ms)))
    return ms.value / n


def probe(lib, nin, nout, doubles):
    from gapflow_amd import _lib
    ms = C.c_double(0.)
    _lib.check(lib.gpf_stream_probe(0, nin, nout, doubles, 10, C.byref(ms)))
    return ms.value


def step_time(o):
    n = o.sizes[0]
    p = build(TEXT.format(n=n, geo=GAPS['2-d']))
    armed = bool(o.arm) and hasattr(p, 'set_statistics')
    if armed:
        p.set_statistics(every=o.arm)
    p._advance(20, honor_stop=False)
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        p._advance(o.step_time, honor_stop=False)
        t.append((time.perf_counter() - t0) * 1e3 / o.step_time)
    print(json.dumps({'root': ROOT, 'n': n, 'armed_stride': o.arm if armed else 0, 'steps_per_call': o.step_time, 'ms_per_step': t}), flush=True)


def main(argv=None):
    cli = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    cli.add_argument('--sizes', type=int, nargs='+', default=[4096])
    cli.add_argument('--steps', type=int, default=20)
    cli.add_argument('--rounds', type=int, default=5)
    cli.add_argument('--step-time', type=int, default=0, metavar='N')
    cli.add_argument('--arm', type=int, default=0, metavar='S')
    cli.add_argument('--json', metavar='FILE')
    o = cli.parse_args(argv)
    if o.step_time:
        return step_time(o)
    out = {'steps': o.steps, 'rounds': o.rounds, 'cases': {}}
    for n in o.sizes:
        p = build(TEXT.format(n=n, geo=GAPS['2-d']))
        doubles = (n + 2) * (n + 2)
        for fields in (('p',), ('p', 'rho', 'jx', 'jy')):
            p.set_statistics(every=1, fields=fields)
            legs = [('off', lambda: timed(p, o.steps, 0)), ('record', lambda: timed(p, o.steps, 1)), ('stream', lambda: timed(p, o.steps, 2))]
            if len(fields) == 1:
                legs.append(('probe', lambda: probe(p._lib, 5, 4, doubles)))
            t = {k: [] for k, _ in legs}
            for r in range(o.rounds + 1):
                for k, leg in legs:
                    v = leg()
                    if r:
                        t[k].append(v)
            added = [a - b for a, b in zip(t['record'], t['off'])]
            nbytes = doubles * 8 * (2 * 4 * len(fields) + (1 if len(fields) == 1 else 3))      # accumulators read and written, q planes read
            res = {'ms': {k: stats(v) for k, v in t.items()}, 'added_ms_per_record': stats(added), 'bytes_per_record': nbytes,
                   'added_GB_per_s': nbytes / statistics.median(added) / 1e6,
                   'stream_over_added': statistics.median(t['stream']) / statistics.median(added)}
            if 'probe' in t:
                res['probe_over_added'] = statistics.median(t['probe']) / statistics.median(added)
            a = res['added_ms_per_record']
            print(f"{n}^2 fields {','.join(fields):12s}: off {res['ms']['off']['median']:.4f} ms/step   record added {a['median']:.4f} "
                  f"({a['min']:.4f} .. {a['max']:.4f}) ms = {res['added_GB_per_s']:.0f} GB/s   stream {res['ms']['stream']['median']:.4f} "
                  f"({res['ms']['stream']['min']:.4f} .. {res['ms']['stream']['max']:.4f})   stream / added {res['stream_over_added']:.2f}"
                  + (f"   probe {res['ms']['probe']['median']:.4f}, probe / added {res['probe_over_added']:.2f}" if 'probe' in t else ''), flush=True)
            out['cases'][f"{n}^2 {','.join(fields)}"] = res
        del p
    if o.json:
        os.makedirs(os.path.dirname(os.path.abspath(o.json)), exist_ok=True)
        with open(o.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
