"""Command line entry: ``python -m gapflow_amd -i input.yaml`` runs one problem to completion
(same flag as the reference's ``python -m GaPFlow -i``, GaPFlow/__main__.py:28-48).

Several GPUs of one node: start one process per GPU,

    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m gapflow_amd -i input.yaml

and the problem is cut into x-slabs (gapflow_amd/slab.py); rank 0 writes the output.  GPF_SLAB_TRANSPORT=p2p selects the
peer-to-peer mailbox transport instead of one all-gather per step.  `options.domain_series: {integrals: N, extrema: M}` in the
YAML file records the film integrals and the field extrema of the whole domain during such a run (all-gather transport;
integrals.npz / extrema.npz from rank 0); a single-process run ignores the key (its own: options.integrals, options.extrema).

``python -m gapflow_amd -i a.yaml b.yaml c.yaml`` runs several small problems together as an ensemble, one workgroup of one
launch each (gapflow_amd/ensemble.py); every one of them writes what it would write run alone.

``python -m gapflow_amd --restart out/checkpoint.gpf [--output DIR] [--max-it N]`` continues a run from a checkpoint.

``python -m gapflow_amd -i fine.yaml --init-from coarse_out/checkpoint.gpf`` starts a run from the state of a run on another grid
of the same domain, resampled on the device (Problem.init_from; the same as `options.init_from` in the YAML file)."""
import argparse
import os
import sys

from . import Problem


class _InputFiles(argparse.Action):
    """`filename` stays the (first) file, a string as ever; `filenames` holds all of them."""
    def __call__(self, parser, namespace, values, option_string=None):
        namespace.filename, namespace.filenames = values[0], list(values)


def make_parser():
    cli = argparse.ArgumentParser(prog='python -m gapflow_amd',
                                  description="Advance a GaPFlow YAML problem on an MI355X.")
    src = cli.add_mutually_exclusive_group(required=True)
    src.add_argument('-i', '--input', dest='filename', metavar='YAML', nargs='+', action=_InputFiles,
                     help="problem definition; several files: run them together as an ensemble (each must fit the one-workgroup kernel)")
    src.add_argument('--restart', metavar='CHECKPOINT', help="continue the run a checkpoint file was written from (options.checkpoint_freq, "
                     "Problem.save_checkpoint); slab runs: the name without .rankNNN, on the same number of processes")
    cli.add_argument('--output', metavar='DIR', help="with --restart: a new output directory for the continued run (default: the saved run's "
                     "options, with '_restart' appended when they name a fixed directory; frames go into a new sol.nc, history.csv "
                     "continues the saved history)")
    cli.add_argument('--max-it', type=int, metavar='N', help="with --restart: run until step N instead of the saved run's max_it")
    cli.add_argument('--init-from', metavar='CHECKPOINT', help="with one -i file: start from the state of this checkpoint, written by a run on "
                     "another grid of the same domain, resampled onto this grid (overrides options.init_from of the file)")
    cli.add_argument('--device', type=int, default=0, help="HIP device ordinal of a single-process run (default 0)")
    return cli


def restart_overrides(opts):
    """(options, numerics) overrides of Problem.from_checkpoint from the command line.  Without --output a saved run that
    wrote into a fixed directory (use_tstamp: False) continues in `<that directory>_restart`: the old one is not empty."""
    options = {'output': opts.output} if opts.output else None
    if options is None:
        from . import checkpoint
        first = opts.restart if os.path.exists(opts.restart) else checkpoint.rank_path(opts.restart, 0)
        try:
            saved = checkpoint.read_file(first)[0]['inputs']['options']
        except (OSError, ValueError, KeyError):
            saved = None                        # from_checkpoint reports what is wrong with the file
        if saved is not None and not saved.get('use_tstamp', True):
            options = {'output': saved['output'].rstrip('/') + '_restart'}
    numerics = {'max_it': opts.max_it} if opts.max_it is not None else None
    return options, numerics


def main(argv=None):
    cli = make_parser()
    opts = cli.parse_args(argv)
    if opts.restart is None and (opts.output or opts.max_it is not None):
        cli.error("--output and --max-it go with --restart")
    several = len(getattr(opts, 'filenames', None) or []) > 1
    if opts.init_from and (opts.restart or several or int(os.environ.get('WORLD_SIZE', '1')) > 1):
        cli.error("--init-from goes with one -i file in a single-process run")
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        if several:
            cli.error("several -i files run as an ensemble on one GPU; a multi-process (slab) run takes one")
        import torch
        import torch.distributed as dist
        from .slab import SlabProblem
        local = int(os.environ.get('LOCAL_RANK', '0'))
        torch.cuda.set_device(local)
        dist.init_process_group('nccl', device_id=torch.device('cuda', local))
        try:
            if opts.restart:
                options, numerics = restart_overrides(opts)
                SlabProblem.from_checkpoint(opts.restart, device=local, options=options, numerics=numerics).run()
            else:
                SlabProblem.from_yaml(opts.filename, device=local).run()
        finally:
            dist.destroy_process_group()
        return 0
    if opts.restart:
        options, numerics = restart_overrides(opts)
        Problem.from_checkpoint(opts.restart, device=opts.device, options=options, numerics=numerics).run()
    elif several:
        from .ensemble import Ensemble
        Ensemble.from_yaml(opts.filenames, device=opts.device).run()
    elif opts.init_from:
        Problem.from_yaml(opts.filename, device=opts.device, init_from=opts.init_from).run()
    else:
        Problem.from_yaml(opts.filename, device=opts.device).run()
    return 0


if __name__ == "__main__":
    sys.exit(main())
