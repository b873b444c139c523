"""Write rate of k_gap_profiles beside a store-only kernel writing the same bytes, and the end-to-end time of
Problem.gap_profiles (device scratch, copies to the host included).

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/profile_time.py [--n 2048] [--nz 32] [--calls 3] [--json FILE]

Problem.gap_profiles(nz, all nine planes) on an n x n journal bearing (Dowson-Higginson), after one warm-up call; then
gpf_profile_store_probe launches k_profile_store_only on the same grid with the same chunk shape as often as the profile
call launched k_gap_profiles.  The bytes of one launch come from the shapes (planes x levels x rows x (Ny + 2) x 8), so
rocprofv3's mean kernel times of the two turn into write rates; the tool's own wall-clock time of a whole call is
reported separately (it is dominated by the copies to pageable host memory)."""
import argparse
import contextlib
import ctypes as C
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

YAML = """
options: {{silent: True}}
grid: {{Nx: {n}, Ny: {n}, Lx: 0.02, Ly: 0.02, xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], xE_D: 877.7007, xW_D: 877.7007,
       yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P']}}
geometry: {{type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.05}}
numerics: {{CFL: 0.25, adaptive: 1, tol: 1e-9, dt: 1e-10, max_it: 100000}}
properties: {{shear: 0.0794, bulk: 0., EOS: DH, P0: 101325, rho0: 877.7007, C1: 3.5e10, C2: 1.23}}
"""


def chunk_rows(nplanes, nz, width, nrows, scratch_mb):
    """Rows per launch, as gpf_gap_profiles splits a request (api_profiles.inc)."""
    half = max(int(scratch_mb * (1 << 20) / 16.0), nplanes * (width + 1))
    assert nplanes * nz * (width + 1) <= half, 'one row of all levels must fit a half of the scratch here'
    return max(1, min(nrows, (half // (nplanes * nz) - 1) // width))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=2048)
    ap.add_argument('--nz', type=int, default=32)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    from gapflow_amd import Problem, _lib
    with contextlib.redirect_stdout(io.StringIO()):
        p = Problem.from_string(YAML.format(n=a.n))
        p._pre_run()
        for _ in range(3):
            p.update()
    nxg, nyg = p.q.shape[1:]
    nplanes = 9
    mb = float(os.environ.get('GPF_PROFILE_SCRATCH_MB', '256'))
    rows = chunk_rows(nplanes, a.nz, nyg, nxg, mb)
    launches = -(-nxg // rows)
    total_bytes = nplanes * a.nz * nxg * nyg * 8
    res = p.gap_profiles(nz=a.nz)                   # warm-up: first touch of the host pages
    del res
    times = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        res = p.gap_profiles(nz=a.nz)
        times.append(time.perf_counter() - t0)
        del res
    lib = _lib.load()
    ms = C.c_double()
    _lib.check(lib.gpf_profile_store_probe(0, rows * nyg, a.nz, nplanes, launches * (a.calls + 1), C.byref(ms)))
    out = {'grid': [nxg, nyg], 'nz': a.nz, 'planes': nplanes, 'scratch_mb': mb, 'rows_per_launch': rows,
           'launches_per_call': launches, 'bytes_per_full_launch': nplanes * a.nz * rows * nyg * 8,
           'bytes_per_call': total_bytes, 'call_s': times, 'call_s_median': float(np.median(times)),
           'host_rate_GBps': total_bytes / float(np.median(times)) / 1e9,
           'store_probe_ms_per_launch': ms.value,
           'store_probe_TBps': nplanes * a.nz * rows * nyg * 8 / (ms.value * 1e-3) / 1e12}
    print(json.dumps(out))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
