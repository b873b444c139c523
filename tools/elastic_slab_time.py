"""Per-step time of the elastic half-space update: the undivided gpf_elastic_update against the x-slab form on one rank
(gpf_elastic_slab_forward/convolve/finish/apply with a loopback group, i.e. the all-to-alls are plain device copies).

    python tools/elastic_slab_time.py [--n 2048] [--reps 50]

Prints one JSON line per boundary case (free, fully periodic): milliseconds per update of each form and their ratio, and
the bytes the slab form's pack / unpack kernels move per update (read + write), from which a
`rocprofv3 --kernel-trace --stats` run of this script gives their achieved bandwidth (k_els_col_pack, k_els_row_pack,
k_els_unpack)."""
import argparse
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TEXT = """
options: {{silent: True}}
grid: {{Lx: 0.0762, Ly: 0.0762, Nx: {n}, Ny: {n}{bc}}}
geometry: {{type: parabolic, hmin: 2.54e-5, hmax: 5.08e-5, U: 4.57, V: 0.3}}
numerics: {{adaptive: 1, CFL: 0.45, tol: 1e-8, dt: 1.e-10, max_it: 60}}
properties:
    EOS: Bayada
    rho0: 850.
    shear: 0.039
    bulk: 0.
    cl: 1600.
    cv: 352.
    elastic: {{E: 50e09, v: 0.3, alpha_underrelax: 0.05}}
    piezo: {{name: Dukler, shearv: 3.9e-5, rhol: 850., rhov: 0.019}}
"""
FREE = (", xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], xE_D: 850., xW_D: 850., "
        "yS: ['D', 'N', 'N'], yN: ['D', 'N', 'N'], yS_D: 850., yN_D: 850.")


def per_update_ms(torch, fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=2048)
    ap.add_argument('--reps', type=int, default=50)
    a = ap.parse_args()
    import ctypes as C
    import torch
    from gapflow_amd import Problem, _lib
    from gapflow_amd.slab import SlabProblem, LoopbackGroup
    warnings.simplefilter('ignore')
    for case, bc in (('free', FREE), ('periodic', '')):
        text = TEXT.format(n=a.n, bc=bc)
        serial = Problem.from_string(text)
        serial._pre_run()
        serial.update()
        t_und = per_update_ms(torch, lambda: _lib.check(serial._lib.gpf_elastic_update(serial._h)), a.reps)
        del serial
        torch.cuda.synchronize()
        slab = SlabProblem.from_string(text, device=0, dist=LoopbackGroup(0, 1))
        slab.pre_run()
        slab.advance(1)
        gathered = C.c_void_p(slab.driver.gathered.data_ptr())
        t_slab = per_update_ms(torch, lambda: slab._elastic.step(gathered), a.reps)
        P = slab._elastic.plan
        c16 = 16
        nrows, nky, nk, nret = P.fwd[0][1], P.nky, P.ky[0][1], len(P.return_rows(0))
        moved = {'k_els_col_pack': 2 * nrows * nky * c16, 'k_els_row_pack': 2 * nret * nk * c16, 'k_els_unpack': 2 * nret * nky * c16}
        print(json.dumps({'case': case, 'n': a.n, 'fft_grid': list(slab._elastic.host.shape_fft), 'undivided_ms': round(t_und, 4),
                          'slab_world1_ms': round(t_slab, 4), 'ratio': round(t_slab / t_und, 3), 'bytes_per_update': moved}))
        del slab
        torch.cuda.synchronize()


if __name__ == '__main__':
    main()
