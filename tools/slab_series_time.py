"""Cost of the domain series of an x-slab run: ms per record -- partials, all-gather of the series message, folds -- beside the
step's own.

    python tools/slab_series_time.py [--size 4096] [--world 8] [--rank 3] [--steps 50] [--rounds 7] [--json FILE]

One process stands in for rank --rank of --world (gapflow_amd.slab.LoopbackGroup: every peer's contribution to a collective is
this rank's own, so the kernels, the message sizes and the launch sequence are a real rank's; the all-gather is a device copy,
NOT xGMI): one (--size / --world) x --size slab of a --size x --size journal bearing.  Started by torch.distributed.run with
one process per GPU (WORLD_SIZE > 1 in the environment) it times real ranks over RCCL instead and rank 0 reports.

A round is --steps eager steps with both series armed at stride 1, as SlabDriver._recording enqueues them, with HIP events on
the stream between the phases of every step: step (gpf_step_local, all-gather, gpf_step_commit), partials
(gpf_slab_series_local), gather (the series message), folds (gpf_slab_series_fold).  The figures are event times per step, so
they hold whatever the host does between the launches of one phase and not what it does between phases.  One warm-up round is
thrown away, then --rounds rounds; every figure is printed with its median and its whole range.  `unarmed` is the same loop
without the series, the step's own time to hold `step` against."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TEXT = """
options: {{silent: True, write_freq: 1000000}}
grid: {{dx: 1.e-5, dy: 1.e-5, Nx: {n}, Ny: {n}, xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P'], yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P']}}
geometry: {{type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.}}
numerics: {{CFL: 0.5, adaptive: 1, tol: 1e-12, dt: 1e-10, max_it: 100000000}}
properties: {{shear: 0.0794, bulk: 0., EOS: DH, P0: 101325., rho0: 877.7007, C1: 3.5e10, C2: 1.23}}
"""


def stats(v):
    return {'median': statistics.median(v), 'min': min(v), 'max': max(v), 'all': list(v)}


def one_round(slab, torch, n, armed):
    """ms per step of each phase, from events on the current stream"""
    d, s = slab.driver, slab.driver.series
    marks = [[torch.cuda.Event(enable_timing=True) for _ in range(5)] for _ in range(n)]
    base = s.begin() if armed else int(slab.state().step)
    for i in range(n):
        ev = marks[i]
        ev[0].record()
        d.engine.step_local(False)
        d.dist.all_gather_into_tensor(d.gathered, d.message)
        d.engine.commit(d.gathered, False, d.rank_lo, d.rank_hi)
        ev[1].record()
        if armed:
            s.local(base + i + 1)
            ev[2].record()
            d.dist.all_gather_into_tensor(s.gathered, s.message)
            ev[3].record()
            s.fold(base + i + 1)
            ev[4].record()
    d.enqueued += n
    torch.cuda.synchronize()
    if armed:
        assert s.end() == n
    else:
        slab.state()
    names = ('step', 'partials', 'gather', 'folds') if armed else ('step',)
    return {name: sum(ev[k].elapsed_time(ev[k + 1]) for ev in marks) / n for k, name in enumerate(names)}


def main():
    cli = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    cli.add_argument('--size', type=int, default=4096)
    cli.add_argument('--world', type=int, default=8)
    cli.add_argument('--rank', type=int, default=3)
    cli.add_argument('--steps', type=int, default=50)
    cli.add_argument('--rounds', type=int, default=7)
    cli.add_argument('--json')
    opts = cli.parse_args()
    import torch
    from gapflow_amd.slab import LoopbackGroup, SlabProblem
    real = int(os.environ.get('WORLD_SIZE', '1')) > 1
    if real:
        import torch.distributed as dist
        local = int(os.environ.get('LOCAL_RANK', '0'))
        torch.cuda.set_device(local)
        dist.init_process_group('nccl', device_id=torch.device('cuda', local))
        group, device = dist, local
    else:
        group, device = LoopbackGroup(opts.rank, opts.world), 0
    with contextlib.redirect_stdout(io.StringIO()):
        slab = SlabProblem.from_string(TEXT.format(n=opts.size), device=device, dist=group)
        slab.pre_run()
        slab.advance(4)
    legs = {'unarmed': [], 'armed': []}
    for r in range(opts.rounds + 1):                    # alternating legs; round 0 is the warm-up
        for leg in ('unarmed', 'armed'):
            if leg == 'armed':
                slab.set_domain_series(integrals=1, extrema=1)
            res = one_round(slab, torch, opts.steps, leg == 'armed')
            if leg == 'armed':
                slab.clear_domain_series()
            if r > 0:
                legs[leg].append(res)
    out = {'transport': 'rccl' if real else 'loopback (device copy)', 'world': slab.world, 'rank': slab.rank,
           'slab': [slab.layout.nx, opts.size], 'steps_per_round': opts.steps, 'rounds': opts.rounds,
           'device': torch.cuda.get_device_name(device),
           'unarmed_step_ms': stats([x['step'] for x in legs['unarmed']]),
           'armed_ms': {k: stats([x[k] for x in legs['armed']]) for k in ('step', 'partials', 'gather', 'folds')}}
    out['record_ms'] = stats([x['partials'] + x['gather'] + x['folds'] for x in legs['armed']])
    if not real or slab.rank == 0:
        def line(name, s):
            print(f"{name:28s} median {s['median'] * 1e3:9.2f} us   range {s['min'] * 1e3:9.2f} .. {s['max'] * 1e3:9.2f} us")
        print(f"[{out['transport']}] rank {out['rank']} of {out['world']}: slab {out['slab'][0]} x {out['slab'][1]}, "
              f"{opts.rounds} rounds of {opts.steps} steps, per step:")
        line('step alone (unarmed)', out['unarmed_step_ms'])
        for k in ('step', 'partials', 'gather', 'folds'):
            line(f'armed: {k}', out['armed_ms'][k])
        line('record (partials+gather+folds)', out['record_ms'])
        if opts.json:
            with open(opts.json, 'w') as f:
                json.dump(out, f, indent=1)
    if real:
        group.destroy_process_group()


if __name__ == '__main__':
    main()
