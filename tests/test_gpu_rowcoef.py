"""The row-coefficient table of the x-only-gap step kernel changes where eight numbers per row come from, never what they are:
a handle whose k_step2 reads them from the table (the default) and one whose kernel evaluates them itself on every row of every
step (GPF_ROWCOEF_TABLE=0 at gpf_create) compute the same bits -- q with its ghost cells, and every scalar.  Shapes: 37 x 200 (two
strips, uneven row chunks, wrap lanes) and 130 x 126 (one full strip, the ghost column in the next); all-periodic and D/N/N in
x; alternating and fixed sweeps; journal and inclined gaps; Dowson-Higginson and one heavy law (power law: one wave per SIMD);
a two-rank slab run with a periodic seam (seam records of the table, seam weight of the reductions).  The table itself is
downloaded and compared with a fresh device evaluation on the gap planes, row by row."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEPS = 8
PERIODIC_X = "xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P']"
DNN_X = "xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], xE_D: {rho0}, xW_D: {rho_w}"
GAPS = {'journal': 'type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.02',
        'inclined': 'type: inclined, hmax: 6.6e-5, hmin: 1.e-5, U: 50., V: 4.'}
LAWS = {'DH': ('EOS: DH, shear: 0.0794, bulk: 0., rho0: 877.7007', 877.7007, 875.),
        'PL': ('EOS: PL, shear: 1.846e-5, bulk: 0., P0: 101325, rho0: 1.1853, alpha: 0.', 1.1853, 1.18)}
TEXT = """
options: {{silent: True}}
grid: {{Nx: {nx}, Ny: {ny}, dx: 1.e-5, dy: 1.e-5, {bcx}, yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P']}}
geometry: {{{gap}}}
numerics: {{CFL: 0.4, adaptive: 1, MC_order: {mc}, tol: 1.e-12, max_it: 1000}}
properties: {{{law}}}
"""


def text_of(nx, ny, bc, mc, gap, law):
    props, rho0, rho_w = LAWS[law]
    bcx = PERIODIC_X if bc == 'periodic' else DNN_X.format(rho0=rho0, rho_w=rho_w)
    return TEXT.format(nx=nx, ny=ny, bcx=bcx, mc=mc, gap=GAPS[gap], law=props)


@contextlib.contextmanager
def table(on):
    old = os.environ.get('GPF_ROWCOEF_TABLE')
    os.environ['GPF_ROWCOEF_TABLE'] = '1' if on else '0'
    try:
        yield
    finally:
        if old is None:
            os.environ.pop('GPF_ROWCOEF_TABLE', None)
        else:
            os.environ['GPF_ROWCOEF_TABLE'] = old


def scalars_of(sc):
    return {f[0]: np.asarray(getattr(sc, f[0])).tobytes() for f in sc._fields_}


def run(text, on):
    from gapflow_amd import Problem
    with table(on):             # read when the handle is created
        prob = Problem.from_string(text)
        prob._pre_run()
        prob._advance(STEPS, honor_stop=False)
    return prob


def download_table(lib, h, nx, source):
    from gapflow_amd import _lib
    out = np.full((nx + 2 + 4, 8), np.nan)
    _lib.check(lib.gpf_row_coefficients(h, source, _lib.as_dp(out), out.size))
    return out


CASES = [(37, 200, 'periodic', 0, 'journal', 'DH'), (37, 200, 'dnn', 1, 'inclined', 'DH'),
         (130, 126, 'periodic', 1, 'journal', 'DH'), (130, 126, 'dnn', 0, 'inclined', 'DH'),
         (37, 200, 'dnn', 0, 'journal', 'PL'), (130, 126, 'periodic', 1, 'inclined', 'PL')]


@pytest.mark.parametrize('nx,ny,bc,mc,gap,law', CASES, ids=['-'.join(map(str, c)) for c in CASES])
def test_table_and_in_kernel_coefficients_give_the_same_bits(hiplib, nx, ny, bc, mc, gap, law):
    text = text_of(nx, ny, bc, mc, gap, law)
    off = run(text, False)
    note_off = off._lib.gpf_plan_note(off._h).decode()
    q_off, s_off, step_off = off.q.copy(), scalars_of(off._scalars()), off.step
    del off
    on = run(text, True)
    note_on = on._lib.gpf_plan_note(on._h).decode()
    assert 'row coefficients evaluated in the kernel' in note_off and 'row coefficients from the table' in note_on, (note_off, note_on)
    assert on.step == STEPS and step_off == STEPS
    q_on = on.q
    assert q_on.shape == (3, nx + 2, ny + 2)
    assert np.isfinite(q_on).all()
    assert q_on.tobytes() == q_off.tobytes(), f'max |difference| {np.abs(q_on - q_off).max():.3e}'
    s_on = scalars_of(on._scalars())
    for name in s_off:
        assert s_on[name] == s_off[name], name


@pytest.mark.parametrize('gap', ['journal', 'inclined'])
def test_table_holds_the_device_evaluation_of_every_row(hiplib, gap):
    """The table against row_coefficients evaluated afresh on the device from column 1 of the gap planes, bit for bit, before and
    after a second upload of another gap; a handle without seams holds zeros in the seam records; a handle created with
    GPF_ROWCOEF_TABLE=0 has no table."""
    from gapflow_amd import Problem, _lib
    nx, ny = 37, 200
    with table(True):
        prob = Problem.from_string(text_of(nx, ny, 'periodic', 0, gap, 'DH'))
        prob._pre_run()
    first = download_table(prob._lib, prob._h, nx, 0)
    assert first.tobytes() == download_table(prob._lib, prob._h, nx, 1).tobytes()
    assert np.isfinite(first).all() and len(np.unique(first[:nx + 2, 3])) > nx // 2      # S0 = -hx / h: another value in (nearly) every row
    assert not first[nx + 2:].any()
    # another gap through the same handle: the table follows the upload
    topo = np.empty((3, nx + 2, ny + 2))
    _lib.check(prob._lib.gpf_download(prob._h, _lib.FIELD_TOPO, _lib.as_dp(topo), topo.size))
    topo[0] *= 1.25
    topo = _lib.f64c(topo)
    _lib.check(prob._lib.gpf_upload(prob._h, _lib.FIELD_TOPO, _lib.as_dp(topo), topo.size))
    second = download_table(prob._lib, prob._h, nx, 0)
    assert second.tobytes() == download_table(prob._lib, prob._h, nx, 1).tobytes()
    assert np.count_nonzero(second[:nx + 2, 3] != first[:nx + 2, 3]) > nx // 2
    with table(False):
        plain = Problem.from_string(text_of(nx, ny, 'periodic', 0, gap, 'DH'))
        plain._pre_run()
    out = np.zeros((nx + 2 + 4, 8))
    assert plain._lib.gpf_row_coefficients(plain._h, 0, _lib.as_dp(out), out.size) != 0


def slab_run(text, on):
    import torch
    from gapflow_amd import _lib
    from gapflow_amd.slab import SlabProblem, ThreadWorld

    def rank_body(group):
        slab = SlabProblem.from_string(text, device=0, dist=group)
        slab.pre_run()
        slab.advance(STEPS)
        st = slab.state()
        sc = _lib.GpfScalars()
        _lib.check(slab.lib.gpf_scalars(slab._h, C.byref(sc)))
        tab = download_table(slab.lib, slab._h, slab.layout.nx, 0) if on else None
        fresh = download_table(slab.lib, slab._h, slab.layout.nx, 1) if on else None
        return slab.layout, slab.local_q(), scalars_of(st), scalars_of(sc), tab, fresh

    with table(on):
        return ThreadWorld(2, torch).run(rank_body)


def test_two_slabs_with_a_periodic_seam_give_the_same_bits(hiplib):
    from gapflow_amd.slab import HALO_SEAM, HALO_NEIGHBOUR
    text = text_of(150, 70, 'periodic', 0, 'journal', 'DH')
    off = slab_run(text, False)
    on = slab_run(text, True)
    assert [(r[0].kind_lo, r[0].kind_hi) for r in on] == [(HALO_SEAM, HALO_NEIGHBOUR), (HALO_NEIGHBOUR, HALO_SEAM)]
    for a, b in zip(off, on):
        assert a[1].tobytes() == b[1].tobytes(), f'rank {a[0].rank}: max |difference| {np.abs(a[1] - b[1]).max():.3e}'
        for k in (2, 3):
            for name in a[k]:
                assert a[k][name] == b[k][name], (a[0].rank, name)
        assert b[4].tobytes() == b[5].tobytes()
    # the seam records are the far slab's rows: rank 0's low edge sees rank 1's last row and outer row, rank 1's high edge rank
    # 0's first row and outer row (the partner row first, then its upwind neighbour)
    (L0, _, _, _, t0, _), (L1, _, _, _, t1, _) = on
    n0, n1 = L0.nx + 2, L1.nx + 2
    assert t0[n0].tobytes() == t1[L1.nx].tobytes() and t0[n0 + 1].tobytes() == t1[L1.nx + 1].tobytes()
    assert t1[n1 + 2].tobytes() == t0[1].tobytes() and t1[n1 + 3].tobytes() == t0[0].tobytes()
    assert not t0[n0 + 2:].any() and not t1[n1:n1 + 2].any()
