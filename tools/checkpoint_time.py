"""Cost of a checkpoint: k_ckpt_pack beside the stream probe, and gpf_checkpoint_save / gpf_checkpoint_load beside plain
downloads of the same bytes.

    python tools/checkpoint_time.py [--n 4096] [--runs 7] [--json FILE]                  # this library
    GPF_LIB_PATH=<parent's .so> python tools/checkpoint_time.py --downloads-only ...     # the parent commit's downloads

An n x n problem, fixed-form closures, x-only (inclined) gap, three steps so that the handle holds a previous state: the blob
then has nine planes (q, the previous q, the gap).  After one warm-up each, the median of --runs runs of
  * gpf_checkpoint_pack_probe: one pass of k_ckpt_pack over the three planes of q (HIP events), beside
    gpf_stream_probe(3 planes in, 3 out, the same number of doubles) in the same process;
  * the whole gpf_checkpoint_save and the whole gpf_checkpoint_load (wall clock, host buffer allocated and touched before);
  * gpf_download of q, q again and the gap: nine planes, the bytes of the blob, through the library's plain path.
--downloads-only stops after the downloads and uses nothing a library without checkpoints lacks, so the same script times the
parent commit's library (GPF_LIB_PATH); alternate the two processes when comparing."""
import argparse
import contextlib
import ctypes as C
import io
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

YAML = """
options: {{silent: True}}
grid: {{Nx: {n}, Ny: {n}, Lx: 0.02, Ly: 0.02, xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], xE_D: 877.7007, xW_D: 877.7007,
       yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P']}}
geometry: {{type: inclined, hmax: 1.2e-5, hmin: 4.e-6, U: 0.5, V: 0.}}
numerics: {{CFL: 0.4, adaptive: 1, tol: 1e-14, dt: 1e-10, max_it: 100000}}
properties: {{EOS: DH, shear: 0.0794, bulk: 0., rho0: 877.7007}}
"""


def median_ms(fn, runs):
    fn()                                    # warm-up
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), t


def main(argv=None):
    cli = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    cli.add_argument('--n', type=int, default=4096)
    cli.add_argument('--runs', type=int, default=7)
    cli.add_argument('--downloads-only', action='store_true')
    cli.add_argument('--json', metavar='FILE')
    o = cli.parse_args(argv)
    from gapflow_amd import Problem, _lib
    if o.downloads_only:                    # a library from before the checkpoint calls: do not ask it for them
        for name in [k for k in _lib.SIGNATURES if k.startswith('gpf_checkpoint')]:
            del _lib.SIGNATURES[name]
    with contextlib.redirect_stdout(io.StringIO()):
        p = Problem.from_string(YAML.format(n=o.n))
        p._pre_run()
        p._advance(3, honor_stop=False)
    lib, h = p._lib, p._h
    plane = (o.n + 2) * (o.n + 2)
    out = {'n': o.n, 'runs': o.runs, 'library': _lib.LIB_PATH, 'plane_MB': plane * 8 / 1e6}

    q, topo = np.zeros((3, o.n + 2, o.n + 2)), np.zeros((3, o.n + 2, o.n + 2))

    def downloads():
        _lib.check(lib.gpf_download(h, _lib.FIELD_Q, _lib.as_dp(q), q.size))
        _lib.check(lib.gpf_download(h, _lib.FIELD_Q, _lib.as_dp(q), q.size))
        _lib.check(lib.gpf_download(h, _lib.FIELD_TOPO, _lib.as_dp(topo), topo.size))
    out['downloads_9_planes_ms'], out['downloads_all_ms'] = median_ms(downloads, o.runs)

    if not o.downloads_only:
        size = C.c_size_t(0)
        _lib.check(lib.gpf_checkpoint_size(h, C.byref(size)))
        blob = np.zeros(size.value, dtype=np.uint8)
        out['blob_MB'], out['blob_planes'] = size.value / 1e6, round(size.value / (plane * 8))

        def save():
            _lib.check(lib.gpf_checkpoint_save(h, blob.ctypes.data_as(C.c_void_p), blob.size, None))

        def load():
            _lib.check(lib.gpf_checkpoint_load(h, blob.ctypes.data_as(C.c_void_p), blob.size))
        out['save_ms'], out['save_all_ms'] = median_ms(save, o.runs)
        out['load_ms'], out['load_all_ms'] = median_ms(load, o.runs)
        out['save_over_downloads'] = out['save_ms'] / out['downloads_9_planes_ms']
        ms = C.c_double(0.)
        pack, probe = [], []
        for _ in range(o.runs):             # alternating, each call with its own warm-up pass inside the library
            _lib.check(lib.gpf_checkpoint_pack_probe(h, 10, C.byref(ms)))
            pack.append(ms.value)
            _lib.check(lib.gpf_stream_probe(0, 3, 3, plane, 10, C.byref(ms)))
            probe.append(ms.value)
        out['pack_3_planes_ms'], out['stream_probe_3in_3out_ms'] = statistics.median(pack), statistics.median(probe)
        out['pack_all_ms'], out['probe_all_ms'] = pack, probe
        out['pack_GBps'] = 2 * 3 * plane * 8 / out['pack_3_planes_ms'] / 1e6
        out['pack_rate_over_probe'] = out['stream_probe_3in_3out_ms'] / out['pack_3_planes_ms']
    line = json.dumps(out)
    print(line)
    if o.json:
        with open(o.json, 'w') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
