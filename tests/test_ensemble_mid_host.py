"""Host side of the ensembles' workspace tier (gapflow_amd/ensemble.py: member_tier, workspace_bytes): no GPU, no library call."""
import pytest

# (Nx, Ny), cells with ghosts, tier: both sides of the LDS limit (1200 cells: 150 KB at 16 doubles) and of MID_GRID_MAX_CELLS
BOUNDARIES = [((100, 1), 306, 'lds'), ((38, 28), 1200, 'lds'), ((39, 28), 1230, 'workspace'), ((126, 126), 16384, 'workspace'),
              ((127, 126), 16512, None), ((200, 200), 40804, None)]


@pytest.mark.parametrize('shape, cells, tier', BOUNDARIES)
def test_tier_boundaries(shape, cells, tier):
    from gapflow_amd.ensemble import member_tier
    assert (shape[0] + 2) * (shape[1] + 2) == cells
    assert member_tier(*shape) == tier
    assert member_tier(shape[1], shape[0]) == tier          # the cell count decides, not the orientation


def test_limits_the_host_plans_with():
    from gapflow_amd import _lib
    assert (_lib.MID_GRID_MAX_CELLS, _lib.MID_GRID_DOUBLES_PER_CELL) == (16384, 19)
    assert _lib.SMALL_GRID_LDS_BYTES // (8 * _lib.SMALL_GRID_DOUBLES_PER_CELL) == 1200
    for name in ('gpf_ensemble_create2', 'gpf_ensemble_limits2', 'gpf_ensemble_member_info'):
        assert name in _lib.SIGNATURES, name


@pytest.mark.parametrize('shape', [s for s, _, t in BOUNDARIES if t == 'workspace'] + [(50, 50), (20, 270), (100, 100), (41, 41)])
def test_workspace_bytes(shape):
    from gapflow_amd.ensemble import workspace_bytes
    cells = (shape[0] + 2) * (shape[1] + 2)
    b = workspace_bytes(*shape)
    assert b % 256 == 0 and 19 * 8 * cells <= b < 19 * 8 * cells + 256


class _Bare:
    """What _refusal reads of a Problem, without a device."""
    def __init__(self, nx, ny):
        from types import SimpleNamespace
        self._gp_models, self.has_gp_model, self._elastic = [], False, None
        self._cfg, self.topo = SimpleNamespace(thinning=0), SimpleNamespace(elastic=False)
        self.grid, self._shape = {'Nx': nx, 'Ny': ny}, (nx + 2, ny + 2)
        self._integral_every = self._probe_cells = self._extrema_every = None


def test_refusal_follows_the_tiers(monkeypatch):
    """A 2-D member up to 126 x 126 is taken; a larger one is refused by name, with the grid, LDS and the new limit."""
    from gapflow_amd.ensemble import _refusal
    monkeypatch.delenv('GPF_SMALL_GRID', raising=False)
    for nx, ny in ((100, 1), (50, 50), (100, 100), (126, 126)):
        assert _refusal(_Bare(nx, ny)) is None
    for nx, ny in ((127, 126), (200, 200)):
        cls, why = _refusal(_Bare(nx, ny))
        assert cls is NotImplementedError and f"{nx} x {ny}" in why and 'LDS' in why and '16384' in why
        assert why.index(f"{nx} x {ny}") < why.index('LDS')


def test_tier_argument_is_checked_before_anything_else():
    from gapflow_amd import Ensemble
    with pytest.raises(ValueError, match="tier"):
        Ensemble([], tier='hbm')
