"""Problem driver with the reference's API surface, running its hot path on an MI355X.

Mirrors GaPFlow/problem.py (reference): ``Problem.from_yaml / from_string / _from_dict``,
``run``, ``_pre_run``, ``update``, the scalar properties and the ``pressure`` /
``wall_stress_xz`` / ``wall_stress_yz`` / ``bulk_stress`` / ``topo`` members the reference's
tests touch.  All per-step arithmetic happens in libgapflow_hip.so (HIP kernels, fp64); this
module only keeps the host-side bookkeeping of problem.py:368-451 and 616-637.

Host <-> device coherence of ``q``: the reference hands out a writable NumPy view
(problem.py:314-317) and its tests assign into it (tests/test_wave_decay.py:101).  Here ``q``
is a host mirror: reading the property downloads the device field if a step ran since the
last read; before the next device operation the mirror is compared with what was downloaded
and uploaded again if the user changed it.
"""
import ctypes as C
import io as _io
import os
import signal
from collections import deque, namedtuple
from datetime import datetime

import numpy as np

from . import _lib
from . import __version__
from .io import read_yaml_input, write_yaml, create_output_directory, history_to_csv
from .series import (ALL_SERIES, SERIES, SERIES_STAGEWISE, _Series, _thinning_series_stride, _changes_stride, _domain_series_entry, _elastic_series_stride, _extrema_stride, _integral_records, _integral_sections,  # noqa: F401
                     _integral_stride, _line_centre, _line_entries, _line_span, _lines_stride, _probe_cells, _region_entries,
                     _regions_stride, _statistics_fields, _statistics_stride, _stride, _weight_planes, _weighted_stride,
                     _frame_axes, _frame_shape, _frame_spec, _frame_window, _frames_stride)
from .topography import Topography
from .stress import Pressure, WallStress, BulkStress

GapProfiles = namedtuple('GapProfiles', 'z u v tau')
GapProfiles.__doc__ = """Through-gap profiles of Problem.gap_profiles: z, u, v (nz, nrows, Ny+2), tau (6, nz, nrows, Ny+2); None if not asked for."""
ProbeSeries = namedtuple('ProbeSeries', 'step time cells rho jx jy p')
ProbeSeries.__doc__ = """Time series of Problem.probes: step, time (nrecords,), cells (nprobes, 2), rho, jx, jy, p (nrecords, nprobes); p None if not asked for."""
FilmIntegrals = namedtuple('FilmIntegrals', ('step', 'time') + _lib.INTEGRAL_SUMS + ('flow_x', 'flow_y', 'sections_x', 'sections_y'))
FilmIntegrals.__doc__ = """Time series of Problem.integrals: step, time and the nine area integrals (nrecords,), flow_x (nrecords, len(sections_x)), flow_y (nrecords, len(sections_y)), the sections' interior rows / columns."""
WeightedIntegrals = namedtuple('WeightedIntegrals', ('step', 'time', 'names') + _lib.WEIGHTED_INTEGRANDS)
WeightedIntegrals.__doc__ = """Time series of Problem.weighted_integrals: step, time (nrecords,), names (the K weight planes'), and per integrand an array (nrecords, K)."""
RegionSeries = namedtuple('RegionSeries', ('step', 'time', 'names') + _lib.WEIGHTED_INTEGRANDS + ('cells', 'area', 'bbox'))
RegionSeries.__doc__ = """Time series of Problem.regions: step, time (nrecords,), names (the K regions'), per integrand an array (nrecords, K), cells (nrecords, K) int64, area = cells dx dy, bbox (nrecords, K, 4) = (ix_min, ix_max, iy_min, iy_max), -1 for an empty region."""
FieldExtrema = namedtuple('FieldExtrema', ('step', 'time') + _lib.EXTREMA_NAMES + ('cells', 'index'))
FieldExtrema.__doc__ = """Time series of Problem.extrema: step, time and the seven values (nrecords,), cells (nrecords, 7, 2) -- (ix, iy) of each value in the ghosted index space --, index: name -> position along the cells' second axis."""
ElasticSeries = namedtuple('ElasticSeries', ('step', 'time') + _lib.ELASTIC_SERIES_NAMES + ('cells',))
ElasticSeries.__doc__ = """Time series of Problem.elastic_series: step, time, the four sums and d_max, d_min (nrecords,), cells (nrecords, 2, 2) -- (ix, iy) of d_max, then of d_min, in the ghosted index space."""
ThinningSeries = namedtuple('ThinningSeries', ('step', 'time') + _lib.THINNING_SERIES_NAMES + ('cells',))
ThinningSeries.__doc__ = """Time series of Problem.thinning_series: step, time, the eleven sums and eta_min, eta_max, rate_max (nrecords,), cells (nrecords, 3, 2) -- (ix, iy) of eta_min, then of eta_max, then of rate_max, in the ghosted index space."""
StepChanges = namedtuple('StepChanges', ('step', 'time') + _lib.CHANGE_NAMES + ('cells', 'index'))
StepChanges.__doc__ = """Time series of Problem.changes: step, time and the eleven values (nrecords,), cells (nrecords, 3, 2) -- (ix, iy) of dmax_rho, dmax_jx, dmax_jy in the ghosted index space --, index: name of a maximum -> position along the cells' second axis."""


def _film_series(rec, sx, sy):
    """FilmIntegrals of the records the _Series `rec` holds, taken with the flow sections sx, sy (Problem's and an Ensemble member's)."""
    ns = len(_lib.INTEGRAL_SUMS)
    data = rec.stacked(0, (ns + len(sx) + len(sy),))
    return FilmIntegrals(rec.step_array(), rec.time_array(), *[data[:, k] for k in range(ns)], data[:, ns:ns + len(sx)],
                         data[:, ns + len(sx):], np.array(sx, dtype=np.int64), np.array(sy, dtype=np.int64))


def _extrema_series(rec):
    """FieldExtrema of the records the _Series `rec` holds (Problem's and a SlabProblem's domain series)."""
    nq = len(_lib.EXTREMA_NAMES)
    vals = rec.stacked(0, (nq,))
    return FieldExtrema(rec.step_array(), rec.time_array(), *[vals[:, k] for k in range(nq)], rec.stacked(1, (nq, 2), np.int32),
                        {name: k for k, name in enumerate(_lib.EXTREMA_NAMES)})


def _probe_series(rec, cells, pressure):
    """ProbeSeries of the records the _Series `rec` holds, taken at `cells` with or without p (Problem's and an Ensemble member's)."""
    nv = 4 if pressure else 3
    data = rec.stacked(0, (len(cells), nv))
    return ProbeSeries(rec.step_array(), rec.time_array(), cells.copy(), data[:, :, 0], data[:, :, 1], data[:, :, 2], data[:, :, 3] if nv == 4 else None)


def _save_probe_series(outdir, series):
    """probes.npz of a ProbeSeries (no p where none was asked for)"""
    np.savez(os.path.join(outdir, 'probes.npz'), **{k: v for k, v in series._asdict().items() if v is not None})


def _save_film_series(outdir, series):
    """integrals.npz of a FilmIntegrals"""
    np.savez(os.path.join(outdir, 'integrals.npz'), **series._asdict())


def _save_extrema_series(outdir, series):
    """extrema.npz of a FieldExtrema: its arrays and `names`, the order along the cells' second axis"""
    s = series._asdict()
    index = s.pop('index')
    np.savez(os.path.join(outdir, 'extrema.npz'), names=np.array(sorted(index, key=index.get)), **s)


def _termination_signals():
    # utils.py:80-95 of the reference
    names = ('SIGINT', 'SIGTERM', 'SIGHUP', 'SIGUSR1')
    return [getattr(signal, n) for n in names if hasattr(signal, n)]


class Problem:
    """Gap-averaged lubrication problem advanced by the fused MacCormack HIP kernel."""

    def __init__(self, options, grid, numerics, prop, geo, gp=None, database=None, extra_field=None, device=0,
                 elastic_on_device=True):
        """elastic_on_device=False: an elastic gap is flagged (topo.nc gets a frame with every solution frame) but not
        deformed here -- the caller supplies the deformed gap (the output writer of gapflow_amd/slab.py)."""
        if gp is not None and database is None:
            raise IOError("GP closures need a training database (`db` section)")
        if database is not None and not getattr(database, 'has_mock_md', True):
            prop['shear'] = 0.                       # problem.py:110-113
            prop['bulk'] = 0.
        self.options, self.grid, self.numerics, self.geo, self.prop = options, grid, numerics, geo, prop
        self.has_gp_model = gp is not None
        self._lib = _lib.require_device()
        Nx, Ny = grid['Nx'], grid['Ny']
        self._shape = (Nx + 2, Ny + 2)

        # device problem
        self._cfg = self._make_config(device)
        self._h = C.c_void_p()
        _lib.check(self._lib.gpf_create(C.byref(self._cfg), C.byref(self._h)))

        # uniform initial state (problem.py:662-670)
        self.step = None
        self._q_host = np.empty((3,) + self._shape)
        self._q_host[0] = prop['rho0']
        self._q_host[1] = prop['rho0'] * geo['U'] / 2.0
        self._q_host[2] = prop['rho0'] * geo['V'] / 2.0
        self._q_snapshot = None
        self._device_newer = False
        self._upload(_lib.FIELD_Q, self._q_host)
        self._q_snapshot = self._q_host.copy()

        # extra field = slip length by default (problem.py:132-135)
        self._extra = np.zeros((1,) + self._shape)
        if extra_field is not None:
            self._extra[...] = extra_field
            self._upload(_lib.FIELD_EXTRA, self._extra)

        self.topo = Topography(grid, geo, prop, on_change=self._upload_topo)
        self._upload_topo()
        self._elastic = None
        if self.topo.elastic and elastic_on_device:         # topography.py:236-249
            from .elastic import ElasticDeformation
            el = prop['elastic']
            self._elastic = ElasticDeformation(el['E'], el['v'], el['alpha_underrelax'], grid, el['n_images'])
            self._elastic.attach(self)
            self.topo.refresh = self._download_topo

        self._closures_stale = True
        self.database = database
        self._gp_models = {}
        if gp is not None:
            from .gp import attach_surrogates
            self._gp_models = attach_surrogates(self, gp, database)
        self.pressure = Pressure(self, self._gp_models.get('zz'))
        self.bulk_stress = BulkStress(self)
        self.wall_stress_xz = WallStress(self, 'x', self._gp_models.get('xz'))
        self.wall_stress_yz = WallStress(self, 'y', self._gp_models.get('yz'))

        sc = self._scalars()
        self._kinetic_energy_old = sc.ekin         # problem.py:670
        self._ekin_old_user = None
        self._stop = False
        self.history = {k: [] for k in ('step', 'time', 'ekin', 'residual', 'vsound')}
        self._restart_history = None            # from_checkpoint: the saved run's history, which run() continues
        self._has_extra_field = extra_field is not None
        self._probe_cells = None
        if options.get('probes') is not None:       # options.probes (from the YAML text, or carried by a checkpoint's dictionaries)
            self.set_probes(options['probes'], pressure=bool(options.get('probes_pressure', True)))
        self._integral_every = None
        if options.get('integrals') is not None:    # options.integrals (from the YAML text, or carried by a checkpoint's dictionaries)
            self.set_integrals(options['integrals'], options.get('integrals_sections_x'), options.get('integrals_sections_y'))
        self._weighted_every = None
        if options.get('weighted_integrals'):       # options.weighted_integrals / options.weights (from the YAML text, or a checkpoint's dictionaries); 0: off
            from . import weights as _weights
            if not options.get('weights'):
                raise ValueError("options.weighted_integrals: options.weights must list the weight planes")
            planes, names = _weights.from_entries(grid, options['weights'])
            self.set_weighted_integrals(planes, options['weighted_integrals'], names)
        self._regions_every = None
        if options.get('regions'):                  # options.regions / options.region_list (from the YAML text, or a checkpoint's dictionaries); 0: off
            if not options.get('region_list'):
                raise ValueError("options.regions: options.region_list must list the regions")
            self.set_regions(options['region_list'], options['regions'])
        self._lines_every = None
        if options.get('lines'):                    # options.lines / options.line_list (from the YAML text, or a checkpoint's dictionaries); 0: off
            if not options.get('line_list'):
                raise ValueError("options.lines: options.line_list must list the lines")
            self.set_lines(options['line_list'], options['lines'])
        self._extrema_every = None
        if options.get('extrema'):                  # options.extrema (from the YAML text, or carried by a checkpoint's dictionaries); 0: off
            self.set_extrema(options['extrema'])
        self._elastic_series_every = None
        if options.get('elastic_series'):           # options.elastic_series (from the YAML text, or carried by a checkpoint's dictionaries); 0: off
            self.set_elastic_series(options['elastic_series'])
        self._thinning_series_every = None
        if options.get('thinning_series'):          # options.thinning_series (from the YAML text, or carried by a checkpoint's dictionaries); 0: off
            self.set_thinning_series(options['thinning_series'])
        self._frames_every, self._frames_nc = None, None
        if options.get('frames'):                   # options.frames / options.frame_spec (from the YAML text, or a checkpoint's dictionaries); 0: off
            self.set_frames(options['frames'], **(options.get('frame_spec') or {}))
        self._changes_every = None
        if options.get('changes'):                 # options.changes (from the YAML text, or carried by a checkpoint's dictionaries); 0: off
            self.set_changes(options['changes'])
        self._stats_every = None
        if options.get('statistics'):               # options.statistics (from the YAML text, or carried by a checkpoint's dictionaries); 0: off
            self.set_statistics(options['statistics'], options.get('statistics_fields', _lib.STATS_FIELDS), options.get('statistics_after', 0))

        if options.get('init_from'):                # options.init_from (from the YAML text, or --init-from): start from another grid's state
            self.init_from(options['init_from'])

        if not options['silent']:
            self.outdir = create_output_directory(options['output'], options['use_tstamp'])
            if database is not None:            # problem.py:158-164: MD datasets go below the run's output directory
                database.set_training_path(os.path.join(self.outdir, 'train'), check_temporary=True)
                database.output_path = self.outdir
                options['output'] = self.outdir
            full = {'version': __version__}
            for k, v in zip(['options', 'grid', 'numerics', 'geo', 'prop'], [options, grid, numerics, geo, prop]):
                full[k] = v
            if database is not None:            # problem.py:175-178
                full['gp'], full['db'], full['md'] = gp, database.config, database.md_config
            write_yaml(full, os.path.join(self.outdir, 'config.yml'))
            from .output import FieldWriter
            self._writer = FieldWriter(self)

    def __del__(self):
        h = getattr(self, '_h', None)
        if h is not None and h.value:
            self._lib.gpf_destroy(h)
            h.value = None

    # -------------------------------------------------------------------------------------
    # constructors (problem.py:211-308)
    # -------------------------------------------------------------------------------------
    @classmethod
    def from_yaml(cls, fname, device=0, init_from=None):
        """init_from: a checkpoint to start from (see ``init_from``), in place of the file's own `options.init_from`; a relative
        path in the FILE is relative to the file, one given here to the working directory."""
        print(f"Reading input file: {fname}")
        with open(fname, "r") as f:
            return cls.from_string(f.read(), device=device, init_from=init_from, base_dir=os.path.dirname(os.path.abspath(fname)))

    @classmethod
    def from_string(cls, ymlstring, device=0, init_from=None, base_dir=None):
        with _io.StringIO(ymlstring) as f:
            input_dict = read_yaml_input(f)
        _keep_own_options(input_dict, ymlstring, base_dir)
        if init_from is not None:
            input_dict['options']['init_from'] = os.path.abspath(os.fspath(init_from))
        return cls._from_dict(input_dict, device=device)

    @classmethod
    def _from_dict(cls, input_dict, device=0):
        gp = input_dict.get('gp', None)
        db = input_dict.get('db', None)
        database = None
        if db is not None:
            from .gp import make_database
            database = make_database(input_dict, device)
        return cls(input_dict['options'], input_dict['grid'], input_dict['numerics'], input_dict['properties'],
                   input_dict['geometry'], gp=gp, database=database, extra_field=None, device=device)

    # -------------------------------------------------------------------------------------
    # configuration -> C struct
    # -------------------------------------------------------------------------------------
    def _edge_rules(self):
        """Resolve problem.py:676-768 into (rule per component, Dirichlet target) for the four ghost edges.

        Reference quirks kept: the low-x ghost takes the xW value and the high-x ghost the xE value,
        but the low-y ghost takes the *yN* value and the high-y ghost the *yS* value (problem.py:746-754).
        """
        g = self.grid
        # (edge, side whose masks select the assigned rows, side that supplies masks+value of the data)
        table = [(0, 'xE', 'xW'), (1, 'xW', 'xE'), (2, 'yS', 'yN'), (3, 'yN', 'yS')]
        rules, values = [], []
        for _, assign, data in table:
            if all(g[f'bc_{assign}_P']):
                rules.append([_lib.BC_P] * 3)
                values.append(0.0)
                continue
            for t in 'DN':
                if list(g[f'bc_{assign}_{t}']) != list(g[f'bc_{data}_{t}']):
                    raise NotImplementedError("opposite edges must declare the same D/N types per component "
                                              "(the reference's mask/value pairing, problem.py:685-707, breaks otherwise)")
            r = []
            for c in range(3):
                if g[f'bc_{data}_D'][c]:
                    r.append(_lib.BC_D)
                elif g[f'bc_{data}_N'][c]:
                    r.append(_lib.BC_N)
                else:
                    raise NotImplementedError("an edge must be periodic for all components or for none")
            rules.append(r)
            values.append(float(g.get(f'bc_{data}_D_val', 0.0)) if any(g[f'bc_{data}_D']) else 0.0)
        return rules, values

    def _make_config(self, device):
        g, n, p, geo = self.grid, self.numerics, self.prop, self.geo
        cfg = _lib.GpfConfig()
        cfg.Nx, cfg.Ny, cfg.dx, cfg.dy = g['Nx'], g['Ny'], g['dx'], g['dy']
        cfg.U, cfg.V = geo['U'], geo['V']
        cfg.eta, cfg.zeta = p['shear'], p['bulk']
        if p['EOS'] not in _lib.EOS_IDS:
            raise NotImplementedError(f"EOS '{p['EOS']}' needs a surrogate model (gp/db sections)")
        cfg.eos = _lib.EOS_IDS[p['EOS']]
        for i, k in enumerate(_lib.EOS_KEYS[p['EOS']]):
            if k not in p and k not in _lib.EOS_DEFAULTS[p['EOS']]:
                raise TypeError(f"EOS '{p['EOS']}' needs the property '{k}'")
            cfg.eos_par[i] = p.get(k, _lib.EOS_DEFAULTS[p['EOS']].get(k))
        cfg.piezo = 0
        if 'piezo' in p and p['piezo']['name'] in _lib.PIEZO_IDS:
            name = p['piezo']['name']
            cfg.piezo = _lib.PIEZO_IDS[name]
            for i, k in enumerate(_lib.PIEZO_KEYS[name]):
                cfg.piezo_par[i] = p['piezo'][k]
        cfg.thinning = 0
        if 'thinning' in p and p['thinning']['name'] in _lib.THINNING_IDS:
            name = p['thinning']['name']
            cfg.thinning = _lib.THINNING_IDS[name]
            for i, k in enumerate(_lib.THINNING_KEYS[name]):
                cfg.thinning_par[i] = p['thinning'][k]
        rules, values = self._edge_rules()
        for e in range(4):
            for c in range(3):
                cfg.bc_rule[e][c] = rules[e][c]
            cfg.bc_value[e] = values[e]
        cfg.halo_lo = cfg.halo_hi = 0
        cfg.adaptive = int(bool(n['adaptive']))
        cfg.CFL, cfg.dt_fixed, cfg.tol = n['CFL'], n['dt'], n['tol']
        cfg.max_it = n['max_it']
        cfg.mc_order = n['MC_order']
        cfg.device = device
        return cfg

    # -------------------------------------------------------------------------------------
    # host <-> device
    # -------------------------------------------------------------------------------------
    def _upload(self, field, arr):
        a = _lib.f64c(arr)
        _lib.check(self._lib.gpf_upload(self._h, field, _lib.as_dp(a), a.size))

    def _download(self, field, ncomp):
        out = np.empty((ncomp,) + self._shape)
        _lib.check(self._lib.gpf_download(self._h, field, _lib.as_dp(out), out.size))
        return out

    def _upload_topo(self):
        self._upload(_lib.FIELD_TOPO, self.topo.full[:3])
        self._closures_stale = True

    def _download_topo(self, field):
        """Host mirror of the deformed gap: h, dh/dx, dh/dy and the displacement (topography.py:283-305)."""
        field[:3] = self._download(_lib.FIELD_TOPO, 3)
        field[3] = self._download(_lib.FIELD_DEFORMATION, 1)[0]

    def _sync_to_device(self):
        """Push user edits of ``q`` before any device operation."""
        if self._q_snapshot is not None and not self._device_newer:
            if not np.array_equal(self._q_host, self._q_snapshot, equal_nan=True):
                self._upload(_lib.FIELD_Q, self._q_host)
                self._q_snapshot = self._q_host.copy()
                self._closures_stale = True

    def _mark_device_advanced(self):
        """The device field has moved on: the host mirror is stale until `q` is read again.  In the reference `q` is the
        live field, so `q = p.q; p.update(); q[0] *= 1.01` edits the NEW state; here that array still holds the old one
        and the edit could only be dropped or misapplied.  The stale mirror is therefore made read-only -- such an edit
        raises at once -- and the next read of `p.q` hands out a NEW array holding the current state.  (NumPy views keep the
        flag they were created with: a view taken earlier, `rho = p.q[0]`, stays writable, but it aliases the retired array
        and can no longer reach the mirror in use; an edit through it goes nowhere, like an edit of any copy.)"""
        self._device_newer = True
        self._closures_stale = True
        self._q_host.flags.writeable = False

    @property
    def q(self):
        """Full density field (3, Nx+2, Ny+2): rho, jx, jy -- a writable host mirror."""
        if self._device_newer:
            self._q_host = np.empty_like(self._q_host)      # the retired array stays read-only; its old views cannot alias this one
            _lib.check(self._lib.gpf_download(self._h, _lib.FIELD_Q, _lib.as_dp(self._q_host), self._q_host.size))
            self._q_snapshot = self._q_host.copy()
            self._device_newer = False
        return self._q_host

    def _derived(self, field):
        self._sync_to_device()
        if self._closures_stale:
            _lib.check(self._lib.gpf_update_closures(self._h))
            self._closures_stale = False
        return self._download(field, _lib.FIELD_NCOMP[field])

    def _scalars(self):
        self._sync_to_device()
        sc = _lib.GpfScalars()
        _lib.check(self._lib.gpf_scalars(self._h, C.byref(sc)))
        return sc

    # -------------------------------------------------------------------------------------
    # scalar properties (problem.py:319-362)
    # -------------------------------------------------------------------------------------
    @property
    def q_has_nan(self):
        return bool(self._scalars().invalid == 1) or bool(np.any(np.isnan(self.q)))

    @property
    def q_has_negative_density(self):
        return bool(np.any(self.q[0] < 0.))

    @property
    def q_is_valid(self):
        return not self.q_has_nan and not self.q_has_negative_density

    @property
    def mass(self):
        return np.float64(self._scalars().mass)

    @property
    def kinetic_energy(self):
        return np.float64(self._scalars().ekin)

    @property
    def kinetic_energy_old(self):
        if self.step is None:
            return np.float64(self._kinetic_energy_old)
        return np.float64(self._scalars().ekin_old)

    @kinetic_energy_old.setter
    def kinetic_energy_old(self, value):
        self._kinetic_energy_old = float(value)
        if self.step is not None:
            _lib.check(self._lib.gpf_set_ekin_old(self._h, float(value)))

    @property
    def v_max(self):
        return np.float64(self._scalars().v_max)

    @property
    def dt_crit(self):
        sc = self._scalars()
        return min(self.grid['dx'], self.grid['dy']) / (sc.v_max + sc.v_sound)

    @property
    def cfl(self):
        return self.dt / self.dt_crit

    @property
    def converged(self):
        return bool(np.all(np.array(self.residual_buffer) < self.tol))

    # -------------------------------------------------------------------------------------
    # checkpoint and restart (no reference counterpart)
    # -------------------------------------------------------------------------------------
    def _checkpoint_refusal(self):
        if self.has_gp_model or self._gp_models:
            from .checkpoint import NOT_SAVED
            raise NotImplementedError(NOT_SAVED['surrogate'])
        if self.step is None:
            raise RuntimeError("checkpoint: call _pre_run() (or run()) first")

    def save_checkpoint(self, path):
        """Write everything the run needs to continue bit for bit into one file (atomically: path + '.tmp', then os.replace):
        the device's checkpoint blob (gpf_checkpoint_save) behind the sanitised input dictionaries and the host's mirror of the run."""
        from . import checkpoint
        self._checkpoint_refusal()
        self._sync_to_device()
        meta = {'kind': 'problem', 'version': __version__,
                'inputs': checkpoint.input_dicts(self.options, self.grid, self.numerics, self.prop, self.geo),
                'extra_field': bool(self._has_extra_field),
                'mirror': {'step': self.step, 'simtime': self.simtime, 'dt': self.dt, 'residual': self.residual,
                           'residual_buffer': list(self.residual_buffer), 'history': self.history,
                           'kinetic_energy_old': self._kinetic_energy_old}}
        checkpoint.write_file(path, meta, checkpoint.device_blob(self._lib, self._h))

    def load_checkpoint(self, path):
        """Continue from a file of save_checkpoint in THIS problem (after _pre_run): the library refuses a checkpoint of another
        configuration, a truncated or a damaged one with a RuntimeError that names what differs, and the problem stays as it was."""
        from . import checkpoint
        self._checkpoint_refusal()
        try:
            meta, blob = checkpoint.read_file(path)
        except ValueError as e:
            raise RuntimeError(str(e)) from None
        if meta.get('kind') != 'problem':
            raise RuntimeError(f"checkpoint: {path} holds one rank of a slab run (kind '{meta.get('kind')}'); load it with SlabProblem")
        self._sync_to_device()
        checkpoint.load_device_blob(self._lib, self._h, blob)
        self._restore_mirror(meta['mirror'])

    def _restore_mirror(self, m):
        self.step, self.simtime, self.dt, self.residual = int(m['step']), m['simtime'], m['dt'], m['residual']
        self.residual_buffer = deque(m['residual_buffer'], 5)
        self._kinetic_energy_old = m['kinetic_energy_old']
        self.history = {k: list(v) for k, v in m['history'].items()}
        self._restart_history = {k: list(v) for k, v in m['history'].items()}
        self._mark_device_advanced()                        # q and the closures are read from the device again
        if self._has_extra_field:
            self._extra = self._download(_lib.FIELD_EXTRA, 1)
        self._download_topo(self.topo._field)               # the gap as the device holds it (deformed; drawn asperity heights)
        self.topo._stale = False

    @classmethod
    def from_checkpoint(cls, path, device=0, options=None, numerics=None):
        """A new problem that continues the saved one: built from the stored input dictionaries, `_pre_run`, then the blob.
        `options` may override 'output' and 'silent' (and 'use_tstamp', 'write_freq', 'checkpoint_freq'), `numerics` 'max_it' and
        'tol' -- when to stop is not part of the state."""
        from . import checkpoint
        try:
            meta, _ = checkpoint.read_file(path)
        except ValueError as e:
            raise RuntimeError(str(e)) from None
        inp = meta['inputs']
        inp['options'].pop('init_from', None)       # where the saved run started from; the blob brings the state
        for given, allowed, target in ((options, ('output', 'silent', 'use_tstamp', 'write_freq', 'checkpoint_freq'), inp['options']),
                                       (numerics, ('max_it', 'tol'), inp['numerics'])):
            for k, v in (given or {}).items():
                if k not in allowed:
                    raise ValueError(f"from_checkpoint: '{k}' cannot be overridden (only {allowed})")
                target[k] = v
        extra = None
        if meta.get('extra_field'):          # a placeholder that makes the handle allocate the field; the blob brings its values
            extra = np.ones((1, inp['grid']['Nx'] + 2, inp['grid']['Ny'] + 2))
        p = cls(inp['options'], inp['grid'], inp['numerics'], inp['properties'], inp['geometry'], extra_field=extra, device=device)
        p._pre_run()
        p.load_checkpoint(path)
        return p

    def _write_checkpoint(self):
        self.save_checkpoint(os.path.join(self.outdir, 'checkpoint.gpf'))

    # -------------------------------------------------------------------------------------
    # a state from another grid (no reference counterpart)
    # -------------------------------------------------------------------------------------
    def init_from(self, source):
        """Take the state of `source` -- a Problem on another grid of the same domain, or the path of a checkpoint.gpf of one --
        resampled onto this problem's grid, on the device (gpf_resample): bilinear interpolation of rho and of the flow rates
        jx h, jy h over the source's ghosted cells at this grid's cell centres, divided by this problem's own gap; the ghost
        cells then follow this problem's boundary conditions.  A converged coarse run is a start for a fine one that saves
        most of its steps (measured in 1-D only).  Coarsening goes through the same rule and is NOT
        conservative.

        Allowed at any time.  Before the first step the run simply begins from the new state; after steps the run starts
        over at step 0 (`_pre_run`), as it would from a state assigned to ``q``, and the probes', integrals', weighted
        integrals', regions', lines', extrema and thinning series start afresh.  `source` is only read.  A path is loaded into a temporary problem on this problem's device,
        which is destroyed before the call returns.
        ValueError: the domains differ (Lx or Ly by more than 1e-12 relative), or a direction is periodic on one side only.
        NotImplementedError: surrogate closures here, or a SlabProblem as the source."""
        from . import resample
        from .slab import SlabProblem
        if self.has_gp_model or self._gp_models:
            raise NotImplementedError("init_from: this problem's closures are surrogates (resampling does not cover them)")
        if isinstance(source, SlabProblem):
            raise NotImplementedError("init_from: a SlabProblem cannot be a source (gather its state into a Problem)")
        tmp = None
        if isinstance(source, (str, os.PathLike)):
            from . import checkpoint
            path = os.fspath(source)
            try:
                meta, _ = checkpoint.read_file(path)
            except ValueError as e:
                raise RuntimeError(str(e)) from None
            if meta.get('kind') != 'problem':
                raise NotImplementedError(f"init_from: {path} holds one rank of a slab run (kind '{meta.get('kind')}')")
            resample.check_geometry(self.grid, meta['inputs']['grid'])
            source = tmp = Problem.from_checkpoint(path, device=self._cfg.device, options={'silent': True})
        elif not isinstance(source, Problem):
            raise TypeError(f"init_from: a Problem or the path of a checkpoint is required, got {type(source).__name__}")
        if source is self:
            raise ValueError("init_from: a problem cannot be its own source")
        try:
            resample.check_geometry(self.grid, source.grid)
            if source._cfg.device != self._cfg.device:
                raise ValueError(f"init_from: the source lives on device {source._cfg.device}, this problem on device {self._cfg.device}")
            resample.check_axes(self.grid, source.grid)
            source._sync_to_device()
            self._sync_to_device()
            _lib.check(self._lib.gpf_resample(self._h, source._h))
        finally:
            if tmp is not None:
                tmp.__del__()
        self._mark_device_advanced()                        # q and the closures are read from the device again
        if self.step is not None:
            self._pre_run()

    # -------------------------------------------------------------------------------------
    # point probes (no reference counterpart)
    # -------------------------------------------------------------------------------------
    def set_probes(self, cells, pressure=True):
        """Record rho, jx, jy (and p) at `cells` after every committed step, on the device, whichever way the steps are taken
        (`update()`, `run()`, batches of any length): the series is what reading ``q`` after every single step would give,
        bit for bit, without leaving the batched path.

        cells: up to 256 pairs (ix, iy) of the ghosted index space, 0 <= ix <= Nx+1, 0 <= iy <= Ny+1 -- ghost cells are legal,
        that is where boundary conditions show.  pressure: also keep p = eos_pressure(rho), the equation of state applied to
        the COMMITTED density by the device function `models.pressure.eos_pressure` runs -- not the corrector-stage pressure
        that the ``pressure`` member holds after a step.  Not available with a pressure surrogate.
        A step that is rolled back as invalid leaves no record.  Starts a new series (see ``probes``).  Checkpoints do not carry
        the series: a problem restored from one whose options hold `probes` has them armed again and its series begins at
        the restart step."""
        cells = _probe_cells(cells, self._shape)
        if pressure and self._gp_models.get('zz') is not None:
            raise ValueError("probes: pressure=True records the equation of state's pressure; this problem's pressure is a surrogate")
        ix = np.ascontiguousarray(cells[:, 0], dtype=np.int32)
        iy = np.ascontiguousarray(cells[:, 1], dtype=np.int32)
        i32p = C.POINTER(C.c_int32)
        _lib.check(self._lib.gpf_probes_set(self._h, len(cells), ix.ctypes.data_as(i32p), iy.ctypes.data_as(i32p), int(bool(pressure))))
        self._probe_cells, self._probe_pressure, self._probe_rec = cells, bool(pressure), _Series('probes')

    def clear_probes(self):
        """Stop recording and drop the series."""
        if self._probe_cells is not None:
            _lib.check(self._lib.gpf_probes_clear(self._h))
        self._probe_cells = None

    @property
    def probes(self):
        """ProbeSeries(step, time, cells, rho, jx, jy, p) of every step committed since set_probes (or _pre_run), across
        `update()` and `run()` calls; None when no probes are set.  `time` is the simulation time the scalar log holds for
        the same steps; p is None unless pressure was asked for."""
        if self._probe_cells is None:
            return None
        return _probe_series(self._probe_rec, self._probe_cells, self._probe_pressure)

    def _collect_probes(self, entries, before=None):
        """The probe records of the stepping call that returned `entries` (its committed steps' scalar records)."""
        if self._probe_cells is None:
            return

        def read(out, n, first, have):
            _lib.check(self._lib.gpf_probes_read(self._h, _lib.as_dp(out), n, first, have))
        self._probe_rec.collect_every_step(read, entries, (len(self._probe_cells), 4 if self._probe_pressure else 3))

    def _write_probes(self):
        _save_probe_series(self.outdir, self.probes)

    # -------------------------------------------------------------------------------------
    # film integrals (no reference counterpart)
    # -------------------------------------------------------------------------------------
    def _integrals_refusal(self):
        if self.has_gp_model or self._gp_models:
            raise NotImplementedError("integrals: surrogate (GP) closures replace the pressure and wall stress the integrals evaluate")
        if self._cfg.thinning:
            raise NotImplementedError("integrals: shear thinning needs grad p, which the reduction does not model")
        if self.topo.elastic and not self._elastic:
            raise NotImplementedError("integrals: this problem's elastic gap is deformed by its caller, not on the device (not supported)")

    def set_integrals(self, every=1, sections_x=None, sections_y=None):
        """Record whole-film integrals of the committed state after every step whose count is a multiple of `every`, on the
        device, whichever way the steps are taken (`update()`, `run()`, batches of any length).

        Per record, summed over the interior cells and multiplied by dx dy: load = p (the equation of state's pressure of the
        committed density; Dowson-Higginson as the reference writes it, with rho / rho0 divided, so that the sum sits at rounding
        distance from the reference's -- the probes' p may differ from it by 1e-10 of p for a stiff law), load_x, load_y = p x, p y at the cell centres of `topography.create_midpoint_grid`
        (centre of pressure: load_x / load), p_hx, p_hy = p dh/dx, p dh/dy (the pressure's in-plane resultant on the profiled
        wall), tau_xz_bot, tau_yz_bot, tau_xz_top, tau_yz_top = the walls' shear stresses, evaluated on the state with the
        closures' viscosity; and the mass-flow rates flow_x[k] = sum_iy jx h dy on interior row sections_x[k], flow_y[k] =
        sum_ix jy h dx on interior column sections_y[k] (at most 8 each; default: first and last interior row / column).
        These are plain integrals of the named fields: NO sign convention (outward normals, which wall acts on which) is applied.
        The same state gives the same bits whatever the batch size or stride.  On grids small enough for the one-workgroup
        kernel the record is written inside the batch (``integrals_in_batch``): no launch is cut, whatever the stride.
        A step that is rolled back as invalid leaves no record.  Starts a new series (see ``integrals``).  Checkpoints do not
        carry the series: a problem restored from one whose options hold `integrals` has them armed again and its series
        begins at the restart step.  With an elastic gap the record of a step is taken behind the deformation that follows it
        (`update()` and `run()` step such a problem stage-wise): it pairs the committed state with the deformed gap `topo.h`
        shows after that step, bit for bit what ``film_integrals()`` gives then.  Not available with surrogate closures or
        shear thinning."""
        self._integrals_refusal()
        every = _integral_stride(every)
        sx = _integral_sections(sections_x, self.grid['Nx'], 'sections_x')
        sy = _integral_sections(sections_y, self.grid['Ny'], 'sections_y')
        ax, ay = np.array(sx, dtype=np.int32), np.array(sy, dtype=np.int32)
        i32p = C.POINTER(C.c_int32)
        _lib.check(self._lib.gpf_integrals_set(self._h, every, len(sx), ax.ctypes.data_as(i32p), len(sy), ay.ctypes.data_as(i32p)))
        self._integral_every, self._integral_sections, self._integral_rec = every, (sx, sy), _Series('integrals', every)

    def clear_integrals(self):
        """Stop recording and drop the series."""
        if self._integral_every is not None:
            _lib.check(self._lib.gpf_integrals_clear(self._h))
        self._integral_every = None

    @property
    def integrals_in_batch(self):
        """True where the armed film integrals are recorded inside the one-workgroup kernel's batch (small grids), False where
        two launches behind every recorded step write them, and when none are armed."""
        yes = C.c_int(0)
        _lib.check(self._lib.gpf_integrals_in_batch(self._h, C.byref(yes)))
        return bool(yes.value)

    def _integral_layout(self):
        if self._integral_every is not None:
            return self._integral_sections
        return _integral_sections(None, self.grid['Nx'], 'sections_x'), _integral_sections(None, self.grid['Ny'], 'sections_y')

    @property
    def integrals(self):
        """FilmIntegrals(step, time, load, ..., flow_x, flow_y, sections_x, sections_y) of every recorded step since
        set_integrals (or _pre_run), across `update()` and `run()` calls; None when no integrals are armed."""
        if self._integral_every is None:
            return None
        return _film_series(self._integral_rec, *self._integral_sections)

    def film_integrals(self):
        """The same record for the current state, as a dict of the names of ``integrals`` (flow_x, flow_y arrays over the
        sections): bit for bit what a step committing this state would have recorded.  Armed or not (then with the default
        sections).  Reads only."""
        self._integrals_refusal()
        self._sync_to_device()
        sx, sy = self._integral_layout()
        ns = len(_lib.INTEGRAL_SUMS)
        out = np.empty(ns + len(sx) + len(sy))
        _lib.check(self._lib.gpf_integrals_now(self._h, _lib.as_dp(out), out.size))
        res = {name: np.float64(out[k]) for k, name in enumerate(_lib.INTEGRAL_SUMS)}
        res.update(flow_x=out[ns:ns + len(sx)].copy(), flow_y=out[ns + len(sx):].copy(),
                   sections_x=np.array(sx, dtype=np.int64), sections_y=np.array(sy, dtype=np.int64))
        return res

    def _collect_integrals(self, entries, before):
        """The records of the stepping call that took the step count from `before` through `entries` (its committed steps)."""
        if self._integral_every is None:
            return
        sx, sy = self._integral_sections

        def read(b, n, steps, have):
            _lib.check(self._lib.gpf_integrals_read(self._h, _lib.as_dp(b[0]), n, steps, have))
        self._integral_rec.collect(read, entries, before, [((len(_lib.INTEGRAL_SUMS) + len(sx) + len(sy),), np.float64)])

    def _write_integrals(self):
        _save_film_series(self.outdir, self.integrals)

    # -------------------------------------------------------------------------------------
    # weighted film integrals (no reference counterpart)
    # -------------------------------------------------------------------------------------
    def _weighted_refusal(self):
        if self.has_gp_model or self._gp_models:
            raise NotImplementedError("weighted integrals: surrogate (GP) closures replace the pressure and wall stress the integrals evaluate")
        if self._cfg.thinning:
            raise NotImplementedError("weighted integrals: shear thinning needs grad p, which the reduction does not model")
        if self._elastic or self.topo.elastic:
            raise NotImplementedError("weighted integrals: an elastic gap steps stage-wise and deforms between steps (not supported)")

    def set_weighted_integrals(self, weights, every=1, names=None):
        """Record, for each of K <= 8 weight planes, the film's integrals with that weight in front after every step whose count
        is a multiple of `every`, on the device, whichever way the steps are taken (`update()`, `run()`, batches of any length).

        weights: array-like (K, Nx, Ny) or (Nx, Ny) over the INTERIOR cells (row ix of the ghosted field is row ix - 1); ghost
        cells never contribute.  `gapflow_amd.weights` builds the usual ones: `box` (a pad, an asperity, a window), `mode` (one
        Fourier mode), `load` (an .npy file).  names: one per plane, default w0, w1, ...
        Per record and plane, summed over the interior cells and multiplied by dx dy: p (the pressure `load` of ``integrals``
        sums: the plane's load), h, rho_h (the mass in the window), jx_h, jy_h, and tau_xz_bot, tau_yz_bot, tau_xz_top,
        tau_yz_top (the walls' shear stresses as ``integrals`` evaluates them).  Plain integrals: NO sign convention is applied.
        A weight of exactly 1.0 adds the cell's term bit for bit and 0.0 nothing, in the order ``integrals`` adds: a plane of
        ones gives p and the tau_* equal to its load and tau_* in every bit, and the same state gives the same bits whatever
        the batch size or stride.  On grids small enough for the one-workgroup kernel the batch is cut at every recorded step:
        choose a stride there (every=1 costs one launch per step).
        A step that is rolled back as invalid leaves no record.  Starts a new series (see ``weighted_integrals``).  Checkpoints
        do not carry the series: a problem restored from one whose options hold `weighted_integrals` and `weights` has them
        armed again and its series begins at the restart step; weights set from code do not survive a restore.  Not available
        with surrogate closures, shear thinning or an elastic gap."""
        self._weighted_refusal()
        every = _weighted_stride(every)
        planes, names = _weight_planes(weights, names, self.grid['Nx'], self.grid['Ny'])
        ghosted = np.zeros((len(planes),) + self._shape)
        ghosted[:, 1:-1, 1:-1] = planes
        _lib.check(self._lib.gpf_weighted_set(self._h, every, len(planes), _lib.as_dp(ghosted)))
        self._weighted_every, self._weighted_names, self._weighted_rec = every, names, _Series('weighted integrals', every)

    def clear_weighted_integrals(self):
        """Stop recording, drop the series and free the weight planes."""
        if self._weighted_every is not None:
            _lib.check(self._lib.gpf_weighted_clear(self._h))
        self._weighted_every = None

    @property
    def weighted_integrals(self):
        """WeightedIntegrals(step, time, names, p, h, rho_h, ...) of every recorded step since set_weighted_integrals (or
        _pre_run), across `update()` and `run()` calls: one array (nrecords, K) per integrand; None when none are armed."""
        if self._weighted_every is None:
            return None
        rec, nq = self._weighted_rec, len(_lib.WEIGHTED_INTEGRANDS)
        data = rec.stacked(0, (len(self._weighted_names), nq))
        return WeightedIntegrals(rec.step_array(), rec.time_array(), tuple(self._weighted_names), *[data[:, :, k] for k in range(nq)])

    def film_weighted(self):
        """The same record for the current state, as {integrand: array(K)}: bit for bit what a step committing this state would
        have recorded.  Needs armed weights (they live on the device).  Reads only."""
        self._weighted_refusal()
        if self._weighted_every is None:
            raise RuntimeError("film_weighted: no weights are set (set_weighted_integrals)")
        self._sync_to_device()
        out = np.empty((len(self._weighted_names), len(_lib.WEIGHTED_INTEGRANDS)))
        _lib.check(self._lib.gpf_weighted_now(self._h, _lib.as_dp(out), out.size))
        return {name: out[:, k].copy() for k, name in enumerate(_lib.WEIGHTED_INTEGRANDS)}

    def _collect_weighted(self, entries, before):
        """The records of the stepping call that took the step count from `before` through `entries` (its committed steps)."""
        if self._weighted_every is None:
            return

        def read(b, n, steps, have):
            _lib.check(self._lib.gpf_weighted_read(self._h, _lib.as_dp(b[0]), n, steps, have))
        self._weighted_rec.collect(read, entries, before, [((len(self._weighted_names), len(_lib.WEIGHTED_INTEGRANDS)), np.float64)])

    def _write_weighted(self):
        s = self.weighted_integrals._asdict()
        s['names'] = np.array(s['names'])
        np.savez(os.path.join(self.outdir, 'weighted.npz'), **s)

    # -------------------------------------------------------------------------------------
    # region series (no reference counterpart)
    # -------------------------------------------------------------------------------------
    def _regions_refusal(self):
        if self.has_gp_model or self._gp_models:
            raise NotImplementedError("regions: surrogate (GP) closures replace the pressure and wall stress the regions evaluate")
        if self._cfg.thinning:
            raise NotImplementedError("regions: shear thinning needs grad p, which the reduction does not model")
        if self._elastic or self.topo.elastic:
            raise NotImplementedError("regions: an elastic gap steps stage-wise and deforms between steps (not supported)")

    def set_regions(self, regions, every=1):
        """Record, for each of K <= 8 regions, what the part of the film in a given state carries after every step whose count
        is a multiple of `every`, on the device, whichever way the steps are taken (`update()`, `run()`, batches of any length).

        regions: a list of dicts {field, above=-inf, below=+inf, box=None, name=None}.  field: 'p' (the equation of state's
        pressure of the committed density: a probe's p, the extrema's), 'rho', 'h', 'jx' or 'jy'.  An interior cell belongs iff
        above <= f < below for its value f -- `above` is inclusive, `below` exclusive, a NaN never belongs -- and it lies in
        box = (ix0, ix1, iy0, iy1), inclusive 1-based interior indices (None: the whole interior).  The zone follows the state
        of each step: {field: 'rho', below: rho_cav} is the cavitated zone, {field: 'h', below: c} the thin film.  names
        default to r0, r1, ...
        Per record and region: the nine sums of ``weighted_integrals`` (p, h, rho_h, jx_h, jy_h, tau_xz_bot, tau_yz_bot,
        tau_xz_top, tau_yz_top) over the region's cells times dx dy -- on a finite state bit for bit what
        `set_weighted_integrals` gives for the 0 / 1 plane of the same predicate --, `cells`, the exact number of member
        cells, `area` = cells dx dy, and `bbox` = (ix_min, ix_max, iy_min, iy_max) over them: (-1, -1, -1, -1) for an empty
        region, whose sums are +0.0.  A zone that wraps a periodic seam reports the full extent along that axis.
        On grids small enough for the one-workgroup kernel the batch is cut at every recorded step: choose a stride there.
        A step that is rolled back as invalid leaves no record.  Starts a new series (see ``regions``).  Checkpoints do not
        carry the series: a problem restored from one whose options hold `regions` and `region_list` has them armed again and
        its series begins at the restart step; regions set from code do not survive a restore.  Not available with surrogate
        closures, shear thinning or an elastic gap."""
        self._regions_refusal()
        every = _regions_stride(every)
        entries = _region_entries(regions, self.grid['Nx'], self.grid['Ny'])
        arr = (_lib.GpfRegion * len(entries))()
        for r, e in zip(arr, entries):
            r.field, r.lo, r.hi = _lib.REGION_FIELDS.index(e['field']), e['above'], e['below']
            r.box[:] = e['box'] if e['box'] is not None else (1, self.grid['Nx'], 1, self.grid['Ny'])
        _lib.check(self._lib.gpf_regions_set(self._h, every, len(entries), arr))
        self._regions_every, self._regions_names, self._regions_rec = every, [e['name'] for e in entries], _Series('regions', every)

    def clear_regions(self):
        """Stop recording, drop the series and free the device buffers."""
        if self._regions_every is not None:
            _lib.check(self._lib.gpf_regions_clear(self._h))
        self._regions_every = None

    def _region_shapes(self):
        """(trailing shape, dtype) of a record's sums and of its integers"""
        K = len(self._regions_names)
        return [((K, len(_lib.WEIGHTED_INTEGRANDS)), np.float64), ((K, len(_lib.REGION_INTS)), np.int64)]

    def _region_record(self, steps, times, sums, ints):
        nq = len(_lib.WEIGHTED_INTEGRANDS)
        cells = ints[:, :, 0].copy()
        return RegionSeries(steps, times, tuple(self._regions_names), *[sums[:, :, k] for k in range(nq)], cells,
                            cells * (self.grid['dx'] * self.grid['dy']), ints[:, :, 1:].copy())

    @property
    def regions(self):
        """RegionSeries(step, time, names, p, h, rho_h, ..., cells, area, bbox) of every recorded step since set_regions (or
        _pre_run), across `update()` and `run()` calls: one array (nrecords, K) per integrand, cells and area (nrecords, K),
        bbox (nrecords, K, 4); None when none are armed."""
        if self._regions_every is None:
            return None
        rec, (sums, ints) = self._regions_rec, self._region_shapes()
        return self._region_record(rec.step_array(), rec.time_array(), rec.stacked(0, *sums), rec.stacked(1, *ints))

    def film_regions(self):
        """The same record for the current state, as {name: array(K)} for the nine integrands, `cells` and `area`, and
        `bbox` (K, 4): bit for bit what a step committing this state would have recorded.  Needs armed regions.  Reads only."""
        self._regions_refusal()
        if self._regions_every is None:
            raise RuntimeError("film_regions: no regions are set (set_regions)")
        self._sync_to_device()
        K = len(self._regions_names)
        sums = np.empty((1, K, len(_lib.WEIGHTED_INTEGRANDS)))
        ints = np.zeros((1, K, len(_lib.REGION_INTS)), dtype=np.int64)
        _lib.check(self._lib.gpf_regions_now(self._h, _lib.as_dp(sums), ints.ctypes.data_as(C.POINTER(C.c_int64)), K))
        rec = self._region_record(None, None, sums, ints)._asdict()
        return {k: v[0].copy() for k, v in rec.items() if k not in ('step', 'time', 'names')}

    def _collect_regions(self, entries, before):
        """The records of the stepping call that took the step count from `before` through `entries` (its committed steps)."""
        if self._regions_every is None:
            return

        def read(b, n, steps, have):
            _lib.check(self._lib.gpf_regions_read(self._h, _lib.as_dp(b[0]), b[1].ctypes.data_as(C.POINTER(C.c_int64)), n, steps, have))
        self._regions_rec.collect(read, entries, before, self._region_shapes())

    def _write_regions(self):
        s = self.regions._asdict()
        s['names'] = np.array(s['names'])
        np.savez(os.path.join(self.outdir, 'regions.npz'), **s)

    # -------------------------------------------------------------------------------------
    # line profiles (viz/plotting.py:51-60, viz/animations.py:200-242 draw them from written frames)
    # -------------------------------------------------------------------------------------
    def _lines_refusal(self):
        if self.has_gp_model or self._gp_models:
            raise NotImplementedError("lines: surrogate (GP) closures replace the pressure and wall stress the lines evaluate")
        if self._cfg.thinning:
            raise NotImplementedError("lines: shear thinning needs grad p, which the recording does not model")
        if self._elastic or self.topo.elastic:
            raise NotImplementedError("lines: an elastic gap steps stage-wise and deforms between steps (not supported)")

    def _line_structs(self, entries):
        arr = (_lib.GpfLine * len(entries))()
        for l, e in zip(arr, entries):
            l.along = _lib.LINE_AXES.index(e['along'])
            l.i0, l.i1 = _line_span(e, self.grid['Nx'], self.grid['Ny'])
        return arr

    def _line_lengths(self, entries):
        return [self.grid['Nx'] if e['along'] == 'x' else self.grid['Ny'] for e in entries]

    def _line_doubles(self, entries):
        return len(_lib.LINE_FIELDS) * sum(self._line_lengths(entries))

    def _line_split(self, data, entries):
        """{name: {field: array(n, length)}} of records (n, doubles of a record) in the library's layout: per line, nine fields,
        each `length` doubles."""
        out, at, nf = {}, 0, len(_lib.LINE_FIELDS)
        for e, length in zip(entries, self._line_lengths(entries)):
            block = data[:, at:at + nf * length].reshape(len(data), nf, length)
            out[e['name']] = {f: block[:, k].copy() for k, f in enumerate(_lib.LINE_FIELDS)}
            at += nf * length
        return out

    def set_lines(self, lines, every=1, capacity=None):
        """Record profiles of the committed state along grid lines after every step whose count is a multiple of `every`, on the
        device, whichever way the steps are taken (`update()`, `run()`, batches of any length): the centre lines that the
        reference's `plot_frame(dim=1)` and animations draw from written frames, or any other row / column, or the mean over a
        band of them -- a journal bearing's circumferential pressure profile at mid-width, or averaged over the width.

        lines: a list of 1 to 8 dicts {along, at=None, name=None}.  along 'x': a profile over the interior rows ix = 1..Nx
        (length Nx), at column `at` (an int iy), or the arithmetic mean over the columns iy0..iy1 inclusive for at = (iy0, iy1);
        1-based interior indices as in the `box` of regions, 1 <= iy0 <= iy1 <= Ny.  at=None is the reference's centre line,
        column (Ny + 2) // 2: `q[:, 1:-1, ny // 2]` of the ghosted array.  along 'y': the same with the axes exchanged (length
        Ny, row ix or rows ix0..ix1, default row (Nx + 2) // 2).  Names default to l0, l1, ...
        Per point nine fields: rho, jx, jy (the state's own bits), p (the equation of state's pressure of the committed density,
        bit for bit a probe's p), h (the gap the device holds), tau_xz_bot, tau_yz_bot, tau_xz_top, tau_yz_top (the walls' shear
        stresses as ``integrals`` evaluates them).  A band adds in a fixed order and divides once: the same state
        gives the same bits whatever the batch size, stride or kernel that stepped.
        capacity: the records the device buffer holds (None: as many as fit 64 MiB, or GPF_LINES_MB MiB; at least 1).  A batch
        never holds more steps than leave that many records, so a small capacity costs launches' latency, nothing else.  On grids
        small enough for the one-workgroup kernel the batch is also cut at every recorded step: choose a stride there.
        A step that is rolled back as invalid leaves no record.  Starts a new series (see ``lines``).  Checkpoints do not carry
        the series: a problem restored from one whose options hold `lines` and `line_list` has them armed again and its series
        begins at the restart step; lines set from code do not survive a restore.  Not available with surrogate closures, shear
        thinning or an elastic gap."""
        self._lines_refusal()
        every = _lines_stride(every)
        if capacity is not None and (isinstance(capacity, (bool, np.bool_)) or not isinstance(capacity, (int, np.integer)) or capacity < 1):
            raise ValueError(f"lines: capacity must be an integer >= 1 (None: the default), got {capacity!r}")
        entries = _line_entries(lines, self.grid['Nx'], self.grid['Ny'])
        _lib.check(self._lib.gpf_lines_set(self._h, every, len(entries), self._line_structs(entries), 0 if capacity is None else int(capacity)))
        self._lines_every, self._lines_entries, self._lines_rec = every, entries, _Series('lines', every)

    def clear_lines(self):
        """Stop recording, drop the series and free the device buffers."""
        if self._lines_every is not None:
            _lib.check(self._lib.gpf_lines_clear(self._h))
        self._lines_every = None

    @property
    def lines(self):
        """The series of every recorded step since set_lines (or _pre_run), across `update()` and `run()` calls: a dict with
        `step`, `time` (nrecords,), `names` (the lines', in order) and per line name a dict of the nine arrays (nrecords, length):
        rho, jx, jy, p, h, tau_xz_bot, tau_yz_bot, tau_xz_top, tau_yz_top.  None when no lines are armed."""
        if self._lines_every is None:
            return None
        rec = self._lines_rec
        out = {'step': rec.step_array(), 'time': rec.time_array(), 'names': tuple(e['name'] for e in self._lines_entries)}
        out.update(self._line_split(rec.stacked(0, (self._line_doubles(self._lines_entries),)), self._lines_entries))
        return out

    def film_lines(self, lines=None):
        """The same record for the current state, as {name: {field: array(length)}}: bit for bit what a step committing this
        state would have recorded.  Of the armed lines, or of `lines` (a list as set_lines takes) without arming anything.
        Reads only."""
        self._lines_refusal()
        if lines is None and self._lines_every is None:
            raise RuntimeError("film_lines: no lines are set (set_lines), and none are given")
        entries = self._lines_entries if lines is None else _line_entries(lines, self.grid['Nx'], self.grid['Ny'])
        self._sync_to_device()
        out = np.empty((1, self._line_doubles(entries)))
        if lines is None:
            _lib.check(self._lib.gpf_lines_now(self._h, 0, None, _lib.as_dp(out), out.size))
        else:
            _lib.check(self._lib.gpf_lines_now(self._h, len(entries), self._line_structs(entries), _lib.as_dp(out), out.size))
        return {name: {f: v[0] for f, v in rec.items()} for name, rec in self._line_split(out, entries).items()}

    def _collect_lines(self, entries, before):
        """The records of the stepping call that took the step count from `before` through `entries` (its committed steps)."""
        if self._lines_every is None:
            return

        def read(b, n, steps, have):
            _lib.check(self._lib.gpf_lines_read(self._h, _lib.as_dp(b[0]), n, steps, have))
        self._lines_rec.collect(read, entries, before, [((self._line_doubles(self._lines_entries),), np.float64)])

    def _write_lines(self):
        """lines.npz: step, time, names, along and at (K, 2: the first and last column / row) of the lines, and `<name>.<field>`
        (nrecords, length) for every line and field."""
        s = self.lines
        arrays = {'step': s['step'], 'time': s['time'], 'names': np.array(s['names']),
                  'along': np.array([e['along'] for e in self._lines_entries]),
                  'at': np.array([_line_span(e, self.grid['Nx'], self.grid['Ny']) for e in self._lines_entries], dtype=np.int64)}
        for name in s['names']:
            arrays.update({f'{name}.{f}': v for f, v in s[name].items()})
        np.savez(os.path.join(self.outdir, 'lines.npz'), **arrays)

    # -------------------------------------------------------------------------------------
    # reduced frames (no reference counterpart: its pictures are drawn from the frames of sol.nc)
    # -------------------------------------------------------------------------------------
    def _frames_refusal(self):
        if self.has_gp_model or self._gp_models:
            raise NotImplementedError("frames: surrogate (GP) closures replace the pressure and wall stress the frames evaluate")
        if self._cfg.thinning:
            raise NotImplementedError("frames: shear thinning needs grad p, which the recording does not model")
        if self._elastic or self.topo.elastic:
            raise NotImplementedError("frames: an elastic gap steps stage-wise and deforms between steps (not supported)")

    def _frame_struct(self, spec):
        s = _lib.GpfFrameSpec()
        s.fields = sum(1 << _lib.FRAME_FIELDS.index(f) for f in spec['fields'])
        s.ix0, s.ix1, s.iy0, s.iy1 = _frame_window(spec, self.grid['Nx'], self.grid['Ny'])
        s.sx, s.sy = spec['stride']
        s.reduce, s.dtype = _lib.FRAME_REDUCE.index(spec['reduce']), _lib.FRAME_DTYPES.index(spec['dtype'])
        return s

    def _frame_bytes(self, spec):
        mx, my = _frame_shape(spec, self.grid['Nx'], self.grid['Ny'])
        return len(spec['fields']) * mx * my * np.dtype(spec['dtype']).itemsize

    def _frame_split(self, data, spec):
        """{field: array(n, mx, my)} of records (n, bytes of a record) in the library's layout: [field in mask order][a][b]."""
        mx, my = _frame_shape(spec, self.grid['Nx'], self.grid['Ny'])
        block = np.ascontiguousarray(data).view(np.dtype(spec['dtype'])).reshape(len(data), len(spec['fields']), mx, my)
        return {f: block[:, k].copy() for k, f in enumerate(spec['fields'])}

    def set_frames(self, every=1, fields=('rho', 'jx', 'jy', 'p'), window=None, stride=(1, 1), reduce='sample', dtype='f4',
                   capacity=None, keep=None):
        """Record reduced frames of the committed state after every step whose count is a multiple of `every`, on the device,
        whichever way the steps are taken (`update()`, `run()`, batches of any length): the picture of the film at a recorded
        step -- few fields, a window, a coarser lattice, single precision -- where a written frame (`write()`) is every derived
        field on the whole ghosted grid in double precision, through the host.

        fields: names out of the lines' nine, with the lines' definitions: rho, jx, jy (the state's own bits), p (the equation of
        state's pressure of the committed density, bit for bit a probe's p), h (the gap the device holds), tau_xz_bot,
        tau_yz_bot, tau_xz_top, tau_yz_top (the walls' shear stresses as ``integrals`` evaluates them -- of the committed state,
        not the corrector-stage closures of `sol.nc`).  A record keeps them in that order.
        window: (ix0, ix1, iy0, iy1), inclusive 1-based interior indices as in the `box` of regions; None: the whole interior.
        stride: (sx, sy), each in 1..64: the window is cut into blocks of sx x sy cells from its corner (ix0, iy0), the last block
        of an axis possibly ragged; a frame is (mx, my) = (ceil(rows / sx), ceil(columns / sy)) values per field.
        reduce: 'sample', the value at the block's first cell (no arithmetic), or 'mean', the arithmetic mean over the block's
        cells inside the window, added in a fixed order and divided once: the same state gives the same bits
        whatever the batch size, stride `every`, capacity or kernel that stepped.  'mean' at stride (1, 1) is 'sample'.
        dtype: 'f4' (the double result converted once, as `astype(float32)` does) or 'f8'.
        capacity: the records the device buffer holds (None: as many as fit 64 MiB, or GPF_FRAMES_MB MiB; at least 1).  A batch
        never holds more steps than leave that many records.  On grids small enough for the one-workgroup kernel the batch is
        also cut at every recorded step: choose a stride there.
        keep: whether the records also stay in memory for ``frames``; None: True for a silent problem, False otherwise -- a
        problem that is not silent appends every collected batch to `frames.nc` in its output directory, and a long run does not
        pile frames up in host memory.
        A step that is rolled back as invalid leaves no record.  Starts a new series (see ``frames``).  Checkpoints do not carry
        the series: a problem restored from one whose options hold `frames` (and `frame_spec`) has it armed again and its series
        begins at the restart step; frames set from code do not survive a restore.  Not available with surrogate closures, shear
        thinning or an elastic gap."""
        self._frames_refusal()
        every = _frames_stride(every)
        spec = _frame_spec({'fields': fields, 'window': window, 'stride': stride, 'reduce': reduce, 'dtype': dtype, 'capacity': capacity},
                           self.grid['Nx'], self.grid['Ny'])
        if keep is not None and not isinstance(keep, (bool, np.bool_)):
            raise ValueError(f"frames: keep must be True, False or None, got {keep!r}")
        _lib.check(self._lib.gpf_frames_set(self._h, every, C.byref(self._frame_struct(spec)), spec['capacity'] or 0))
        self._close_frames_nc()
        self._frames_every, self._frames_spec, self._frames_rec = every, spec, _Series('frames', every)
        self._frames_keep = bool(self.options['silent']) if keep is None else bool(keep)

    def clear_frames(self):
        """Stop recording, drop the series, close `frames.nc` and free the device buffer."""
        if self._frames_every is not None:
            _lib.check(self._lib.gpf_frames_clear(self._h))
            self._close_frames_nc()
        self._frames_every = None

    def _frame_dict(self, spec, arrays, **head):
        nx, ny = self.grid['Nx'], self.grid['Ny']
        x, y = _frame_axes(spec, nx, ny, self.grid['dx'], self.grid['dy'])
        out = dict(head, fields=spec['fields'], window=_frame_window(spec, nx, ny), stride=tuple(spec['stride']), reduce=spec['reduce'], x=x, y=y)
        out.update(arrays)
        return out

    @property
    def frames(self):
        """The series of every recorded step since set_frames (or _pre_run) that was kept in memory (`keep`), across `update()`
        and `run()` calls: a dict with `step`, `time` (nrecords,), `fields`, `window`, `stride`, `reduce` (as recorded: 'mean' at
        stride (1, 1) is 'sample'), `x` (mx,), `y` (my,) -- the cell-centre coordinates of the output points: the first cell's for
        'sample', the mean of the block's cell centres for 'mean' -- and per field an array (nrecords, mx, my) of the chosen
        dtype.  None when no frames are armed."""
        if self._frames_every is None:
            return None
        rec, spec = self._frames_rec, self._frames_spec
        data = rec.stacked(0, (self._frame_bytes(spec),), np.uint8)
        return self._frame_dict(spec, self._frame_split(data, spec), step=rec.step_array(), time=rec.time_array())

    def frame_now(self, **spec):
        """The same record for the current state: bit for bit what a step committing this state would have recorded, as the dict
        of ``frames`` without `step` and `time` and with one (mx, my) array per field.  Of the armed frame (no arguments), or of
        the frame given by set_frames' `fields`, `window`, `stride`, `reduce`, `dtype`, without arming anything.  Reads only."""
        self._frames_refusal()
        if not spec and self._frames_every is None:
            raise RuntimeError("frame_now: no frames are set (set_frames), and no spec is given")
        if spec:
            if 'capacity' in spec or 'keep' in spec or 'every' in spec:
                raise ValueError(f"frame_now: fields, window, stride, reduce and dtype describe a frame, got {sorted(spec)}")
            spec = _frame_spec(spec, self.grid['Nx'], self.grid['Ny'], where='frame_now')
            arg = C.byref(self._frame_struct(spec))
        else:
            spec, arg = self._frames_spec, None
        self._sync_to_device()
        out = np.empty((1, self._frame_bytes(spec)), dtype=np.uint8)
        _lib.check(self._lib.gpf_frames_now(self._h, arg, out.ctypes.data_as(C.c_void_p), out.size))
        return self._frame_dict(spec, {f: v[0] for f, v in self._frame_split(out, spec).items()})

    def _frames_writer(self):
        """frames.nc of a problem that is not silent, opened when the first batch is collected (or the run ends without one)."""
        if self._frames_nc is None:
            from .output import FrameWriter
            spec, nx, ny = self._frames_spec, self.grid['Nx'], self.grid['Ny']
            x, y = _frame_axes(spec, nx, ny, self.grid['dx'], self.grid['dy'])
            self._frames_nc = FrameWriter(os.path.join(self.outdir, 'frames.nc'), spec['fields'], spec['dtype'], x, y,
                                          _frame_window(spec, nx, ny), spec['stride'], spec['reduce'])
        return self._frames_nc

    def _close_frames_nc(self):
        if self._frames_nc is not None:
            self._frames_nc.close()
        self._frames_nc = None

    def _collect_frames(self, entries, before):
        """The records of the stepping call that took the step count from `before` through `entries` (its committed steps): to
        `frames.nc` unless the problem is silent, and to the series in memory if it keeps them."""
        if self._frames_every is None:
            return
        rec, spec = self._frames_rec, self._frames_spec

        def read(b, n, steps, have):
            _lib.check(self._lib.gpf_frames_read(self._h, b[0].ctypes.data_as(C.c_void_p), n, steps, have))
        had = len(rec.blocks)
        rec.collect(read, entries, before, [((self._frame_bytes(spec),), np.uint8)])
        if len(rec.blocks) == had:
            return
        n = len(rec.blocks[-1][0])
        if n and not self.options['silent']:
            self._frames_writer().append(rec.steps[len(rec.steps) - n:], rec.times[len(rec.times) - n:], self._frame_split(rec.blocks[-1][0], spec))
        if not self._frames_keep:
            rec.reset()

    def _write_frames(self):
        """frames.nc is complete: every batch was appended as it was collected."""
        self._frames_writer()
        self._close_frames_nc()

    # -------------------------------------------------------------------------------------
    # field extrema (no reference counterpart)
    # -------------------------------------------------------------------------------------
    def _extrema_refusal(self):
        if self._gp_models.get('zz') is not None:
            raise ValueError("extrema: p_max and p_min are the equation of state's pressure; this problem's pressure is a surrogate")

    def set_extrema(self, every=1):
        """Record where the extremes of the committed state sit after every step whose count is a multiple of `every`, on the
        device, whichever way the steps are taken (`update()`, `run()`, batches of any length, the stage-wise pipeline of
        shear-thinning, elastic and surrogate-shear problems).

        Per record, over the interior cells 1..Nx x 1..Ny, each with its cell (ix, iy) of the ghosted index space: p_max, p_min
        (the equation of state's pressure of the committed density: bit for bit the `p` a probe at that cell records), rho_max,
        rho_min, h_min (the gap the device holds: deformed, for an elastic gap, as `topo.h` shows it after that step), u_max,
        v_max (|jx / rho|, |jy / rho|).  Ties go to the smallest ix, then the smallest iy.  The same state gives the same bits
        whatever the batch size or stride; on grids small enough for the one-workgroup kernel the records are written inside
        the batch, which is not cut.  rho = 0 makes a velocity inf: plain IEEE, not special-cased.
        A step that is rolled back as invalid leaves no record.  Starts a new series (see ``extrema``).  Checkpoints do not
        carry the series: a problem restored from one whose options hold `extrema` has them armed again and its series
        begins at the restart step.  Not available when the pressure is a surrogate."""
        self._extrema_refusal()
        every = _extrema_stride(every, allow_zero=False)
        _lib.check(self._lib.gpf_extrema_set(self._h, every))
        self._extrema_every, self._extrema_rec = every, _Series('extrema', every)

    def clear_extrema(self):
        """Stop recording and drop the series."""
        if self._extrema_every is not None:
            _lib.check(self._lib.gpf_extrema_clear(self._h))
        self._extrema_every = None

    @property
    def extrema(self):
        """FieldExtrema(step, time, p_max, ..., v_max, cells, index) of every recorded step since set_extrema (or _pre_run),
        across `update()` and `run()` calls; None when no extrema are armed.  cells[n, index[name]] is the (ix, iy) of `name`."""
        if self._extrema_every is None:
            return None
        return _extrema_series(self._extrema_rec)

    def field_extrema(self):
        """The same record for the current state, as a dict: the seven names of ``extrema`` and, for each, `<name>_cell` =
        (ix, iy).  Bit for bit what a step committing this state would have recorded.  Armed or not.  Reads only."""
        self._extrema_refusal()
        self._sync_to_device()
        vals = np.empty(len(_lib.EXTREMA_NAMES))
        cells = np.zeros((len(_lib.EXTREMA_NAMES), 2), dtype=np.int32)
        _lib.check(self._lib.gpf_extrema_now(self._h, _lib.as_dp(vals), cells.ctypes.data_as(C.POINTER(C.c_int32))))
        res = {}
        for k, name in enumerate(_lib.EXTREMA_NAMES):
            res[name] = np.float64(vals[k])
            res[name + '_cell'] = (int(cells[k, 0]), int(cells[k, 1]))
        return res

    def _collect_extrema(self, entries, before):
        """The records of the stepping call that took the step count from `before` through `entries` (its committed steps)."""
        if self._extrema_every is None:
            return
        nq = len(_lib.EXTREMA_NAMES)

        def read(b, n, steps, have):
            _lib.check(self._lib.gpf_extrema_read(self._h, _lib.as_dp(b[0]), b[1].ctypes.data_as(C.POINTER(C.c_int32)), n, steps, have))
        self._extrema_rec.collect(read, entries, before, [((nq,), np.float64), ((nq, 2), np.int32)])

    def _write_extrema(self):
        _save_extrema_series(self.outdir, self.extrema)

    # -------------------------------------------------------------------------------------
    # deformation series of an elastic gap (no reference counterpart)
    # -------------------------------------------------------------------------------------
    def _elastic_series_refusal(self):
        if not self._elastic:
            raise NotImplementedError("elastic series: this problem has no elastic gap deformed on the device (properties.elastic)")

    def set_elastic_series(self, every=1):
        """Record how far the wall gives way after every step whose count is a multiple of `every`, on the device, behind the
        deformation that follows the step (an elastic problem steps stage-wise, `update()` and `run()` alike).

        Per record, over the interior cells 1..Nx x 1..Ny, with d the deformation the device holds (what `topo.deformation`
        shows after that step), p the pressure ``integrals`` sums as `load` and h the deformed gap: d_sum (the displaced
        volume), d2_sum (sum of d d: the RMS deflection is sqrt(d2_sum / area)), p_d (sum of p d: twice the elastic work of a
        linear half-space -- the factor 1/2 is yours), h_sum (the film's volume), each summed in the order ``integrals`` adds
        and multiplied by dx dy once; and d_max, d_min with their cells (ix, iy) of the ghosted index space, ties going to the
        smallest ix, then the smallest iy, as in ``extrema``.  The same state, gap and deformation give the same bits whatever
        the stride.  A step that is rolled back as invalid leaves no record.  Starts a new series (see ``elastic_series``).
        Checkpoints do not carry the series: a problem restored from one whose options hold `elastic_series` has it armed again
        and its series begins at the restart step.  May be armed beside every other series an elastic problem accepts.  Not
        available without an elastic gap."""
        self._elastic_series_refusal()
        every = _elastic_series_stride(every, allow_zero=False)
        _lib.check(self._lib.gpf_elastic_series_set(self._h, every))
        self._elastic_series_every, self._elastic_series_rec = every, _Series('elastic series', every)

    def clear_elastic_series(self):
        """Stop recording and drop the series."""
        if self._elastic_series_every is not None:
            _lib.check(self._lib.gpf_elastic_series_clear(self._h))
        self._elastic_series_every = None

    @property
    def elastic_series(self):
        """ElasticSeries(step, time, d_sum, d2_sum, p_d, h_sum, d_max, d_min, cells) of every recorded step since
        set_elastic_series (or _pre_run), across `update()` and `run()` calls; None when the series is not armed.
        cells[n, 0] is the (ix, iy) of d_max, cells[n, 1] that of d_min."""
        if self._elastic_series_every is None:
            return None
        rec, nq = self._elastic_series_rec, len(_lib.ELASTIC_SERIES_NAMES)
        vals = rec.stacked(0, (nq,))
        return ElasticSeries(rec.step_array(), rec.time_array(), *[vals[:, k] for k in range(nq)], rec.stacked(1, (2, 2), np.int32))

    def film_elastic(self):
        """The same record for the current state, gap and deformation, as a dict: the six names of ``elastic_series`` and
        `d_max_cell`, `d_min_cell` = (ix, iy).  Bit for bit what a step leaving them would have recorded.  Armed or not.
        Reads only."""
        self._elastic_series_refusal()
        self._sync_to_device()
        vals = np.empty(len(_lib.ELASTIC_SERIES_NAMES))
        cells = np.zeros((2, 2), dtype=np.int32)
        _lib.check(self._lib.gpf_elastic_series_now(self._h, _lib.as_dp(vals), cells.ctypes.data_as(C.POINTER(C.c_int32))))
        res = {name: np.float64(vals[k]) for k, name in enumerate(_lib.ELASTIC_SERIES_NAMES)}
        res['d_max_cell'] = (int(cells[0, 0]), int(cells[0, 1]))
        res['d_min_cell'] = (int(cells[1, 0]), int(cells[1, 1]))
        return res

    def _collect_elastic_series(self, entries, before):
        """The records of the step that took the step count from `before` through `entries` (its committed step)."""
        if self._elastic_series_every is None:
            return

        def read(b, n, steps, have):
            _lib.check(self._lib.gpf_elastic_series_read(self._h, _lib.as_dp(b[0]), b[1].ctypes.data_as(C.POINTER(C.c_int32)), n, steps, have))
        self._elastic_series_rec.collect(read, entries, before, [((len(_lib.ELASTIC_SERIES_NAMES),), np.float64), ((2, 2), np.int32)])

    def _write_elastic_series(self):
        np.savez(os.path.join(self.outdir, 'elastic_series.npz'), **self.elastic_series._asdict())

    # -------------------------------------------------------------------------------------
    # shear-thinning series (no reference counterpart)
    # -------------------------------------------------------------------------------------
    def _thinning_series_refusal(self):
        if not self._cfg.thinning:
            raise NotImplementedError("thinning series: this problem has no shear thinning (properties.thinning: Eyring or Carreau)")
        if self._gp_models:
            raise NotImplementedError("thinning series: the record evaluates the analytic pressure and wall stress; this problem's closures are surrogates")

    def set_thinning_series(self, every=1):
        """Record what a shear-thinning film carries and what it costs its walls after every step whose count is a multiple of
        `every`, on the device, behind the step (a thinning problem steps stage-wise, `update()` and `run()` alike).

        Per record, over the interior cells 1..Nx x 1..Ny of the committed state, with grad p the central differences of the
        equation of state's pressure over the four neighbours (ghost cells included), mu0 the Newtonian viscosity
        (piezo-viscosity included), rate = models.viscosity.shear_rate_avg(grad p, h, U, V, mu0) and eta = mu0
        shear_thinning_factor(rate, mu0) -- cell by cell what ``wall_stress_xz`` / ``wall_stress_yz`` are made of once the
        closures are refreshed for that state: `load` (the pressure ``integrals`` sums as `load`), tau_xz_bot, tau_yz_bot,
        tau_xz_top, tau_yz_top (the wall shear stresses with eta), tau0_* (the same with mu0: what the film would cost without
        thinning), eta_sum and rate_sum (mean viscosity: eta_sum / area), each summed in the order ``integrals`` adds and
        multiplied by dx dy once; and eta_min, eta_max, rate_max with their cells (ix, iy) of the ghosted index space, ties
        going to the smallest ix, then the smallest iy, as in ``extrema``.  The same state and gap give the same bits whatever
        the stride.  With an elastic gap too the record is taken behind the deformation that follows the step, of the
        deformed gap.  A step that is rolled back as invalid leaves no record.  Starts a new series (see ``thinning_series``).
        Checkpoints do not carry the series: a problem restored from one whose options hold `thinning_series` has it armed
        again and its series begins at the restart step.  May be armed beside probes, extrema and statistics.  Not available
        without shear thinning, nor with surrogate closures."""
        self._thinning_series_refusal()
        every = _thinning_series_stride(every, allow_zero=False)
        _lib.check(self._lib.gpf_thinning_series_set(self._h, every))
        self._thinning_series_every, self._thinning_series_rec = every, _Series('thinning series', every)

    def clear_thinning_series(self):
        """Stop recording and drop the series."""
        if self._thinning_series_every is not None:
            _lib.check(self._lib.gpf_thinning_series_clear(self._h))
        self._thinning_series_every = None

    @property
    def thinning_series(self):
        """ThinningSeries(step, time, load, tau_*, tau0_*, eta_sum, rate_sum, eta_min, eta_max, rate_max, cells) of every
        recorded step since set_thinning_series (or _pre_run), across `update()` and `run()` calls; None when the series is not
        armed.  cells[n, 0] is the (ix, iy) of eta_min, cells[n, 1] that of eta_max, cells[n, 2] that of rate_max."""
        if self._thinning_series_every is None:
            return None
        rec, nq = self._thinning_series_rec, len(_lib.THINNING_SERIES_NAMES)
        vals = rec.stacked(0, (nq,))
        return ThinningSeries(rec.step_array(), rec.time_array(), *[vals[:, k] for k in range(nq)],
                              rec.stacked(1, (len(_lib.THINNING_SERIES_EXTREMA), 2), np.int32))

    def film_thinning(self):
        """The same record for the current state and gap, as a dict: the fourteen names of ``thinning_series`` and
        `eta_min_cell`, `eta_max_cell`, `rate_max_cell` = (ix, iy).  Bit for bit what a step leaving them would have recorded.
        Armed or not.  Reads only."""
        self._thinning_series_refusal()
        self._sync_to_device()
        vals = np.empty(len(_lib.THINNING_SERIES_NAMES))
        cells = np.zeros((len(_lib.THINNING_SERIES_EXTREMA), 2), dtype=np.int32)
        _lib.check(self._lib.gpf_thinning_series_now(self._h, _lib.as_dp(vals), cells.ctypes.data_as(C.POINTER(C.c_int32))))
        res = {name: np.float64(vals[k]) for k, name in enumerate(_lib.THINNING_SERIES_NAMES)}
        for k, name in enumerate(_lib.THINNING_SERIES_EXTREMA):
            res[name + '_cell'] = (int(cells[k, 0]), int(cells[k, 1]))
        return res

    def _collect_thinning_series(self, entries, before):
        """The records of the step that took the step count from `before` through `entries` (its committed step)."""
        if self._thinning_series_every is None:
            return

        def read(b, n, steps, have):
            _lib.check(self._lib.gpf_thinning_series_read(self._h, _lib.as_dp(b[0]), b[1].ctypes.data_as(C.POINTER(C.c_int32)), n, steps, have))
        self._thinning_series_rec.collect(read, entries, before, [((len(_lib.THINNING_SERIES_NAMES),), np.float64),
                                                                  ((len(_lib.THINNING_SERIES_EXTREMA), 2), np.int32)])

    def _write_thinning_series(self):
        np.savez(os.path.join(self.outdir, 'thinning_series.npz'), **self.thinning_series._asdict())

    # -------------------------------------------------------------------------------------
    # step changes (no reference counterpart)
    # -------------------------------------------------------------------------------------
    def _changes_refusal(self):
        if self._gp_models or self._cfg.thinning or self._elastic:
            raise NotImplementedError("changes: surrogate, shear-thinning and elastic problems step stage-wise, which keeps no "
                                      "previous state on the device")

    def set_changes(self, every=1):
        """Record how far each conserved field moved in every step whose count is a multiple of `every`, on the device, behind
        the fused step, whichever way the steps are taken (`update()`, `run()`, batches of any length).

        Per record, over the interior cells 1..Nx x 1..Ny, with d = q(step n) - q(step n - 1) per field: d2_rho, d2_jx, d2_jy
        (sum of d d, times dx dy), q2_rho, q2_jx, q2_jy (sum of q q of the new state, times dx dy: the relative L2 change of a
        field is sqrt(d2 / q2), its rate that over `dt`), dmass (sum of d_rho h dx dy with the gap the device holds: the mass
        defect of the step, well conditioned because d_rho is an (almost always) exact difference), dmax_rho, dmax_jx, dmax_jy
        (the largest |d|, each with its cell (ix, iy) of the ghosted index space, ties going to the smallest ix, then the
        smallest iy) and dt, the step size of that step.  No sign convention, no normalisation; ghost cells never contribute.
        The state before the step is the device's other buffer: nothing is downloaded and batches stay whole; on grids small
        enough for the one-workgroup kernel the batch is cut at every recorded step.  The same two states give the same bits
        whatever the batch size or stride.  A step that is rolled back as invalid leaves no record.  Starts a new series (see
        ``changes``).  Checkpoints do not carry the series: a problem restored from one whose options hold `changes` has it
        armed again and its series begins at the restart step.  Not available on problems that step stage-wise (surrogate
        closures, shear thinning, an elastic gap)."""
        self._changes_refusal()
        every = _changes_stride(every, allow_zero=False)
        _lib.check(self._lib.gpf_changes_set(self._h, every))
        self._changes_every, self._changes_rec = every, _Series('changes', every)

    def clear_changes(self):
        """Stop recording and drop the series."""
        if self._changes_every is not None:
            _lib.check(self._lib.gpf_changes_clear(self._h))
        self._changes_every = None

    @property
    def changes(self):
        """StepChanges(step, time, d2_rho, ..., dt, cells, index) of every recorded step since set_changes (or _pre_run), across
        `update()` and `run()` calls; None when the series is not armed.  cells[n, index[name]] is the (ix, iy) of `name`."""
        if self._changes_every is None:
            return None
        rec, nq, nm = self._changes_rec, len(_lib.CHANGE_NAMES), len(_lib.CHANGE_MAXIMA)
        vals = rec.stacked(0, (nq,))
        return StepChanges(rec.step_array(), rec.time_array(), *[vals[:, k] for k in range(nq)], rec.stacked(1, (nm, 2), np.int32),
                           {name: k for k, name in enumerate(_lib.CHANGE_MAXIMA)})

    def step_change(self):
        """The same record for the current state against the state before the last step, as a dict: the eleven names of
        ``changes`` and `dmax_rho_cell`, `dmax_jx_cell`, `dmax_jy_cell` = (ix, iy).  Bit for bit what that step recorded or
        would have.  Armed or not.  Reads only.  The library's state error (GapflowHipError) when the previous state is not
        on the device: before the first step, after `q` was assigned or `init_from`, after the closures were re-evaluated
        (reading `pressure.pressure` redoes the predictor into that buffer); the next `update()` brings it back."""
        self._changes_refusal()
        self._sync_to_device()
        vals = np.empty(len(_lib.CHANGE_NAMES))
        cells = np.zeros((len(_lib.CHANGE_MAXIMA), 2), dtype=np.int32)
        _lib.check(self._lib.gpf_changes_now(self._h, _lib.as_dp(vals), cells.ctypes.data_as(C.POINTER(C.c_int32))))
        res = {name: np.float64(vals[k]) for k, name in enumerate(_lib.CHANGE_NAMES)}
        for k, name in enumerate(_lib.CHANGE_MAXIMA):
            res[name + '_cell'] = (int(cells[k, 0]), int(cells[k, 1]))
        return res

    def _collect_changes(self, entries, before):
        """The records of the stepping call that took the step count from `before` through `entries` (its committed steps)."""
        if self._changes_every is None:
            return
        nq, nm = len(_lib.CHANGE_NAMES), len(_lib.CHANGE_MAXIMA)

        def read(b, n, steps, have):
            _lib.check(self._lib.gpf_changes_read(self._h, _lib.as_dp(b[0]), b[1].ctypes.data_as(C.POINTER(C.c_int32)), n, steps, have))
        self._changes_rec.collect(read, entries, before, [((nq,), np.float64), ((nm, 2), np.int32)])

    def _write_changes(self):
        s = self.changes._asdict()
        index = s.pop('index')
        np.savez(os.path.join(self.outdir, 'changes.npz'), names=np.array(sorted(index, key=index.get)), **s)

    # -------------------------------------------------------------------------------------
    # running field statistics (no reference counterpart)
    # -------------------------------------------------------------------------------------
    def set_statistics(self, every=1, fields=_lib.STATS_FIELDS, after=0):
        """Keep, on the device, per cell of the ghosted grid the mean, the variance, the smallest and the largest value of `fields`
        -- any of 'p', 'rho', 'jx', 'jy' -- over the committed steps whose count is a multiple of `every` and greater than
        `after`, from now on and whichever way the steps are taken (`update()`, `run()`, batches of any length): the peak-pressure
        map of a start-up, the lowest density every cell reached, the time-mean and fluctuation of an oscillating run, without
        downloading ``q`` after every step.

        'p' is eos_pressure(rho), the equation of state applied to the COMMITTED density by the device function a probe's p uses
        -- not the corrector-stage pressure the ``pressure`` member holds; it is not available with a pressure surrogate
        ('rho', 'jx', 'jy' are).  The statistics are those of the recorded SAMPLE (Welford's update, every operation rounded on
        its own: restating it on downloaded states gives the same bits); nothing is weighted by dt.  A step that is rolled back
        as invalid is not recorded.  A record reads and writes four planes per field: on a large grid choose a stride.
        Starts a new window, as do `_pre_run`, `init_from` and a restored checkpoint (checkpoints do not carry the
        accumulators: a problem restored from one whose options hold `statistics` is armed again and its window begins at the
        restart step)."""
        every, after = _statistics_stride(every, 'statistics', low=1), _statistics_stride(after, 'statistics_after', low=0)
        fields = _statistics_fields(fields)
        if 'p' in fields and self._gp_models.get('zz') is not None:
            raise ValueError("statistics: 'p' is the equation of state's pressure; this problem's pressure is a surrogate")
        mask = sum(1 << _lib.STATS_FIELDS.index(f) for f in fields)
        self._sync_to_device()
        _lib.check(self._lib.gpf_stats_set(self._h, every, after, mask))
        self._stats_every, self._stats_fields, self._stats_after = every, fields, after

    def clear_statistics(self):
        """Stop recording and free the accumulators."""
        if self._stats_every is not None:
            _lib.check(self._lib.gpf_stats_clear(self._h))
        self._stats_every = None

    @property
    def statistics(self):
        """The window since set_statistics (or `_pre_run`), fetched from the device on access: a dict of `count`, `first_step`,
        `last_step`, `t_first`, `t_last` and, per field f, `f_mean`, `f_var` (m2 / count, the population form; zeros at
        count == 1), `f_m2`, `f_min`, `f_max`, each of shape (Nx+2, Ny+2).  None while nothing is armed or recorded."""
        if self._stats_every is None:
            return None
        cnt, first, last = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        t0, t1 = C.c_double(0.), C.c_double(0.)
        _lib.check(self._lib.gpf_stats_info(self._h, C.byref(cnt), C.byref(first), C.byref(last), C.byref(t0), C.byref(t1)))
        if cnt.value == 0:
            return None
        out = {'count': int(cnt.value), 'first_step': int(first.value), 'last_step': int(last.value), 't_first': t0.value, 't_last': t1.value}
        for f in self._stats_fields:
            for k, name in enumerate(_lib.STATS_QUANTITIES):
                a = np.empty(self._shape)
                _lib.check(self._lib.gpf_stats_read(self._h, _lib.STATS_FIELDS.index(f), k, _lib.as_dp(a), a.size))
                out[f'{f}_{name}'] = a
            out[f'{f}_var'] = out[f'{f}_m2'] / out['count']
        return out

    def _write_statistics(self):
        s = self.statistics
        if s is not None:
            np.savez(os.path.join(self.outdir, 'statistics.npz'), fields=np.array(self._stats_fields), **s)

    # -------------------------------------------------------------------------------------
    # run loop (problem.py:368-503)
    # -------------------------------------------------------------------------------------
    def _features(self):
        """(ncell, 7) GP feature matrix of the current state, all cells incl. ghosts (gp.py:223-232)."""
        return np.vstack([self.q, self.topo.full[:3], self._extra]).reshape(7, -1).T

    def _pre_run(self):
        self._sync_to_device()
        if self._gp_models:
            # init_database + init of every surrogate (problem.py:418-424, stress.py:278-287, 586-598)
            self.database.initialize(self._features(), self.grid['dim'])
            for m in self._gp_models.values():
                m.init()
        _lib.check(self._lib.gpf_pre_run(self._h))
        if self._kinetic_energy_old is not None:
            _lib.check(self._lib.gpf_set_ekin_old(self._h, float(self._kinetic_energy_old)))
        sc = self._scalars()
        self.step = 0
        self.simtime = 0.
        self.residual = 1.
        self.residual_buffer = deque([self.residual], 5)
        self.dt = sc.dt
        self.tol = self.numerics['tol']
        self.max_it = self.numerics['max_it']
        for row in ALL_SERIES + SERIES_STAGEWISE:   # the step count starts over: so does every armed series
            if row.recorder is not None and getattr(self, row.marker) is not None:
                getattr(self, row.recorder).reset()

    def _absorb(self, entries):
        """Fold the per-step records of a batch into the host-side mirror of the run state."""
        for e in entries:
            if e.invalid and e.step == self.step:
                continue
            self.residual = e.residual
            self.residual_buffer.append(e.residual)
            self.step = int(e.step)
            self.simtime = e.simtime
            self.dt = e.dt

    def _advance(self, n, honor_stop):
        """Enqueue up to n updates on the device; returns the per-step records that actually ran."""
        self._sync_to_device()
        log = (_lib.GpfScalars * n)()
        nexec = C.c_int64(0)
        before = self.step
        _lib.check(self._lib.gpf_step(self._h, n, int(honor_stop), log, n, C.byref(nexec)))
        return self._absorb_batch(log, n, int(nexec.value) - before, before)

    def _absorb_batch(self, log, n, ran, before):
        """The host's bookkeeping behind a batch of n steps of which `ran` were committed, taking the step count on from `before`;
        log: its n per-step records, zero where none was written (shared with Ensemble, whose members' batches run in one launch)."""
        entries = [log[i] for i in range(ran)]
        self._absorb(entries)
        for row in ALL_SERIES:
            if row.fused:
                getattr(self, row.collect)(entries, before)
        if ran > 0:
            self._mark_device_advanced()
        failed = ran < n and log[ran].invalid != 0 if ran < n else False
        if failed:
            self._finalize(log[ran].invalid)
        return entries

    def update(self):
        """One MacCormack predictor-corrector time step (problem.py:509-569), on the device."""
        if self.step is None:
            raise RuntimeError("call _pre_run() (or run()) before update()")
        if self._gp_models or self._cfg.thinning or self._elastic:
            self._update_with_surrogates()      # stage-wise pipeline (host between stages / grad p for thinning / elastic gap)
        else:
            self._advance(1, honor_stop=False)

    def _update_with_surrogates(self):
        """The same step through the stage-wise pipeline: the host sits between the stages because a
        surrogate may retrain or extend its database there (gp.py:435-506, problem.py:532-560)."""
        self._sync_to_device()
        lib, h = self._lib, self._h
        one_step_before_output = (self.step + 1) % self.options['write_freq'] == 0       # problem.py:530
        feats = None

        def features_of_cell(i):
            nonlocal feats
            if feats is None:
                feats = self._features()        # active learning runs in the predictor only: working field == q
            return feats[i]

        _lib.check(lib.gpf_open_step(h))
        for i in range(2):
            for m in self._gp_models.values():
                m.sync_scales()             # the database may have grown through another model since this one was fitted
            _lib.check(lib.gpf_stage_closures(h))
            changed = False
            for name in ('zz', 'xz', 'yz'):
                m = self._gp_models.get(name)
                if m is not None:
                    changed |= m.stage(i == 0, one_step_before_output, features_of_cell)
            if changed:
                _lib.check(lib.gpf_stage_closures(h))
            _lib.check(lib.gpf_stage_advance(h, i))
        for m in self._gp_models.values():
            m.sync_scales()                 # the sound speed that closes the step sees the current scales too
        sc = _lib.GpfScalars()
        before = self.step
        _lib.check(lib.gpf_close_step(h, C.byref(sc)))
        if sc.invalid:
            self._finalize(sc.invalid)
            return
        if self._elastic:
            # Topography.update (problem.py:566): the gap deforms under the pressure of the last closure evaluation
            # (the corrector's), on the device; the host mirror of the topography is refreshed on access
            _lib.check(lib.gpf_elastic_update(h))
            self.topo.mark_stale()
        self._absorb([sc])
        self._collect_probes([sc])
        self._collect_extrema([sc], before)     # (an elastic gap's record was taken behind gpf_elastic_update, of the deformed gap)
        self._collect_thinning_series([sc], before)     # (likewise)
        if self._elastic:                       # likewise its film integrals and its deformation series
            self._collect_integrals([sc], before)
            self._collect_elastic_series([sc], before)
        self._mark_device_advanced()
        # the derived fields on the device ARE what the reference's field objects hold now: the closures of the corrector stage
        # (problem.py:531-560; neither the averaging nor Topography.update re-evaluates them)
        self._closures_stale = False

    def _finalize(self, reason):
        # problem.py:588-610: the device kept the pre-step field; closures refresh lazily
        print('NaN detected.' if reason == 1 else 'Negative density detected.', end=' ')
        print('Writing previous step and aborting simulation.')
        self._closures_stale = True
        self._stop = True

    def _receive_signal(self, signum, frame):
        if signum in _termination_signals():
            self._stop = True

    def _run_begin(self):
        """What run() does before its first step; returns the steps between checkpoints (0: none).  Shared with Ensemble.run."""
        if self.step is None:
            self._pre_run()
        self._stop = False
        self.history = self._restart_history or {k: [] for k in ('step', 'time', 'ekin', 'residual', 'vsound')}
        self._restart_history = None
        silent = self.options['silent']
        cf = 0 if silent else int(self.options.get('checkpoint_freq', 0) or 0)      # steps between checkpoint.gpf; 0: none
        if not silent:
            print(61 * '-')
            print(f"{'Step':6s} {'Timestep':10s} {'Time':10s} {'CFL':10s} {'Residual':10s}")
            print(61 * '-')
            # (a restarted run's history already ends with the row of the step it starts from)
            self.write(scalars=not (self.history['step'] and self.history['step'][-1] == self.step), params=False)
        return cf

    def _run_active(self):
        return not self.converged and self.step < self.max_it and not self._stop

    def _run_batch_length(self, cf):
        return _batch_length(self.step, self.options['write_freq'], self.max_it, cf)

    def _run_after_batch(self, cf):
        """Frame and checkpoint at this problem's own multiples, after an update or a batch.  Shared with Ensemble.run."""
        if self.step % self.options['write_freq'] == 0 and not self.options['silent'] and not self._stop:
            self.write()
        if cf > 0 and self.step % cf == 0 and not self._stop and not self.converged and self.step < self.max_it:
            self._write_checkpoint()    # (a run that ends here writes its checkpoint once, in _run_end)

    def _run_end(self, cf, keep_open=False):
        if not keep_open:
            self._post_run()
        if cf > 0:
            self._write_checkpoint()            # the state the run ends on, with the history _post_run completed

    def run(self, keep_open=False):
        cf = self._run_begin()
        old = {s: signal.signal(s, self._receive_signal) for s in _termination_signals()} \
            if _in_main_thread() else {}
        self._tic = datetime.now()
        try:
            while (self._gp_models or self._cfg.thinning or self._elastic) and self._run_active():
                self.update()                   # surrogates: one host-driven step at a time
                self._run_after_batch(cf)
            while self._run_active():
                # steps until the next frame (problem.py:404) or max_it, whichever comes first; the
                # device stops by itself at convergence, so a batch never overshoots the reference's loop
                self._advance(self._run_batch_length(cf), honor_stop=True)
                self._run_after_batch(cf)
        finally:
            for s, hdl in old.items():
                signal.signal(s, hdl)
        self._run_end(cf, keep_open)

    def _post_run(self):
        walltime = datetime.now() - self._tic
        silent = self.options['silent']
        if self.step % self.options['write_freq'] != 0 and not silent:
            self.write()
        if not silent:
            self._writer.close()
        speed = self.step / max(walltime.total_seconds(), 1e-12)
        print(33 * '=')
        print("Total walltime   : ", str(walltime).split('.')[0])
        print(f"({speed:.2f} steps/s)")
        for name in ('zz', 'xz', 'yz'):             # problem.py:475-483
            m = self._gp_models.get(name)
            if m is not None:
                print(f" - GP train ({name}) : ", str(m.cumtime_train).split('.')[0])
                print(f" - GP infer ({name}) : ", str(m.cumtime_infer).split('.')[0])
        print(33 * '=')
        if not silent:
            history_to_csv(os.path.join(self.outdir, 'history.csv'), self.history)
            for row in ALL_SERIES + SERIES_STAGEWISE:       # (the statistics last of SERIES, the later series behind them)
                if getattr(self, row.marker) is not None:
                    getattr(self, row.write)()
            for name, m in self._gp_models.items():  # problem.py:490-503
                history_to_csv(os.path.join(self.outdir, f'gp_{name}.csv'), m.history)
                with open(os.path.join(self.outdir, f'gp_{name}.txt'), 'w') as f:
                    print(m, file=f)

    def gap_profiles(self, nz=32, rows=None, fields=('z', 'u', 'v', 'tau'), gradients=False):
        """Velocity and viscous stress across the film of the current state (models/profiles.py on the whole field).

        Evaluates the state ``q`` holds (not the corrector-stage closures of ``wall_stress_*``) on the gap ``topo`` holds
        (deformed, for an elastic gap), at nz levels z_k = h k / (nz - 1) per cell, with the solver's closure branch: slip
        at the upper wall with the slip-length field, the closures' shear viscosity (piezo-viscosity included) and
        zeta = prop['bulk'].  grad q enters only with ``gradients=True`` (np.gradient over the ghosted field / dx, dy).
        ``rows``: a slice of the ghosted x index (default: all Nx + 2).  Returns GapProfiles(z, u, v, tau) with z, u, v of
        shape (nz, nrows, Ny + 2) and tau (6, nz, nrows, Ny + 2) in Voigt order; fields not asked for are None.  Reads only:
        q, the run state and later steps are unchanged."""
        if self._gp_models:
            raise NotImplementedError("gap_profiles: surrogate (GP) closures have no through-gap profile")
        if self._cfg.thinning:
            raise NotImplementedError("gap_profiles: shear thinning needs grad p, which the profile does not model")
        if isinstance(nz, bool) or not isinstance(nz, (int, np.integer)) or nz < 2:
            raise ValueError(f"gap_profiles: nz must be an integer >= 2, got {nz!r}")
        nxg, nyg = self._shape
        rows = slice(None) if rows is None else rows
        if not isinstance(rows, slice) or rows.step not in (None, 1):
            raise ValueError("gap_profiles: rows must be a slice of the ghosted x index with step 1")
        ix0 = 0 if rows.start is None else rows.start
        ix1 = nxg if rows.stop is None else rows.stop
        if not (0 <= ix0 < ix1 <= nxg):
            raise ValueError(f"gap_profiles: rows {ix0}:{ix1} outside 0:{nxg} or empty")
        fields = (fields,) if isinstance(fields, str) else tuple(fields)
        bits = {'z': _lib.PROFILE_Z, 'u': _lib.PROFILE_U, 'v': _lib.PROFILE_V, 'tau': _lib.PROFILE_TAU}
        if not fields or any(f not in bits for f in fields):
            raise ValueError(f"gap_profiles: fields must be taken from {tuple(bits)}, got {fields!r}")
        mask = 0
        for f in fields:
            mask |= bits[f]
        self._sync_to_device()
        names = [f for f in ('z', 'u', 'v', 'tau') if mask & bits[f]]
        nplanes = sum(6 if f == 'tau' else 1 for f in names)
        out = np.empty((nplanes, int(nz), ix1 - ix0, nyg))
        _lib.check(self._lib.gpf_gap_profiles(self._h, int(nz), ix0, ix1, mask, _lib.PROFILE_GRADIENTS if gradients else 0,
                                              out.ctypes.data_as(C.c_void_p)))
        res, k = {}, 0
        for f in names:
            res[f] = out[k:k + 6] if f == 'tau' else out[k]
            k += 6 if f == 'tau' else 1
        return GapProfiles(res.get('z'), res.get('u'), res.get('v'), res.get('tau'))

    def write(self, scalars=True, fields=True, params=True):
        # problem.py:616-637
        if scalars:
            sc = self._scalars()
            cfl = self.dt / (min(self.grid['dx'], self.grid['dy']) / (sc.v_max + sc.v_sound))
            print(f"{self.step:<6d} {self.dt:.4e} {self.simtime:.4e} {cfl:.4e} {self.residual:.4e}")
            self.history["step"].append(self.step)
            self.history["time"].append(self.simtime)
            self.history["ekin"].append(sc.ekin)
            self.history["residual"].append(self.residual)
            self.history["vsound"].append(sc.v_sound)
        if fields and not self.options['silent']:
            self._writer.append_frame()
        if params:
            for m in self._gp_models.values():
                m.write()


def _batch_length(step, write_freq, max_it, checkpoint_freq=0):
    """Steps of the next batch of a run that stands at `step`: up to the next frame (problem.py:404), to max_it, to the next
    checkpoint (checkpoint_freq > 0), and at most what the device log holds -- whichever comes first."""
    n = min(write_freq - step % write_freq, max_it - step, _lib.LOG_CAPACITY)
    return min(n, checkpoint_freq - step % checkpoint_freq) if checkpoint_freq > 0 else n


# This project's own `options` keys.  The sanitiser keeps the reference's keys only (as the reference, which ignores unknown ones),
# so they are read from the YAML text and set beside the sanitised ones -- only when given (checkpoint_freq apart), so that every
# other input's dictionaries stay as they are -- and checked here, on the host.  One function per key family, each taking the
# sanitised dictionaries, the text's `options` mapping and the YAML file's directory.
def _own_checkpoint_freq(input_dict, opts, base_dir):
    """`options.checkpoint_freq`: always written, 0 when absent."""
    input_dict['options']['checkpoint_freq'] = int(opts.get('checkpoint_freq', 0) or 0)


def _own_probes(input_dict, opts, base_dir):
    """`options.probes: [[ix, iy], ...]` and `options.probes_pressure`; the cells are checked against the grid, when the input has one."""
    if opts.get('probes') is not None:
        grid = input_dict.get('grid') or {}
        shape = (int(grid['Nx']) + 2, int(grid['Ny']) + 2) if 'Nx' in grid and 'Ny' in grid else None
        input_dict['options']['probes'] = _probe_cells(opts['probes'], shape).tolist()
        if 'probes_pressure' in opts:
            input_dict['options']['probes_pressure'] = bool(opts['probes_pressure'])


def _own_integrals(input_dict, opts, base_dir):
    """`options.integrals: N` (the stride) and `options.integrals_sections_x / _y`; the sections are checked against the grid, when
    the input has one."""
    if opts.get('integrals') is not None:
        grid = input_dict.get('grid') or {}
        input_dict['options']['integrals'] = _integral_stride(opts['integrals'])
        for key, n in (('integrals_sections_x', 'Nx'), ('integrals_sections_y', 'Ny')):
            if opts.get(key) is not None:
                input_dict['options'][key] = _integral_sections(opts[key], int(grid[n]) if n in grid else 2**31 - 1, key)


def _own_extrema(input_dict, opts, base_dir):
    """`options.extrema: N` (the stride; 0 or absent: off)."""
    if opts.get('extrema') is not None:
        input_dict['options']['extrema'] = _extrema_stride(opts['extrema'])


def _own_domain_series(input_dict, opts, base_dir):
    """`options.domain_series: {integrals: N, extrema: M, sections_x: [...], sections_y: [...]}`: the series a SlabProblem records
    over the whole domain (SlabProblem.set_domain_series); the sections are checked against the grid, when the input has one.  A
    Problem stores the key and never arms it, so that one file serves both."""
    if opts.get('domain_series') is not None:
        grid = input_dict.get('grid') or {}
        input_dict['options']['domain_series'] = _domain_series_entry(opts['domain_series'], grid.get('Nx'), grid.get('Ny'),
                                                                      where='options.domain_series')


def _own_changes(input_dict, opts, base_dir):
    """`options.changes: N` (the stride; 0 or absent: off)."""
    if opts.get('changes') is not None:
        input_dict['options']['changes'] = _changes_stride(opts['changes'])


def _own_elastic_series(input_dict, opts, base_dir):
    """`options.elastic_series: N` (the stride; 0 or absent: off)."""
    if opts.get('elastic_series') is not None:
        input_dict['options']['elastic_series'] = _elastic_series_stride(opts['elastic_series'])


def _own_thinning_series(input_dict, opts, base_dir):
    """`options.thinning_series: N` (the stride; 0 or absent: off)."""
    if opts.get('thinning_series') is not None:
        input_dict['options']['thinning_series'] = _thinning_series_stride(opts['thinning_series'])


def _own_weighted(input_dict, opts, base_dir):
    """`options.weighted_integrals: N` (the stride; 0 or absent: off) and `options.weights: [{box: ...}, {mode: ...}, {file: ...}]`
    (gapflow_amd/weights.py: parse_entries); a `file` becomes an absolute path, relative ones taken from the YAML file's directory."""
    from . import weights as _weights
    if opts.get('weighted_integrals') is not None:
        input_dict['options']['weighted_integrals'] = _weighted_stride(opts['weighted_integrals'], allow_zero=True)
    if opts.get('weights') is not None:
        input_dict['options']['weights'] = _weights.parse_entries(opts['weights'], input_dict.get('grid') or None, base_dir)
    if input_dict['options'].get('weighted_integrals') and not input_dict['options'].get('weights'):
        raise ValueError("options.weighted_integrals: options.weights must list the weight planes")


def _own_statistics(input_dict, opts, base_dir):
    """`options.statistics: N` (the stride; 0 or absent: off), `options.statistics_fields: [p, rho]` and `options.statistics_after: M`."""
    if opts.get('statistics') is not None:
        input_dict['options']['statistics'] = _statistics_stride(opts['statistics'], 'statistics', low=0)
    if opts.get('statistics_fields') is not None:
        input_dict['options']['statistics_fields'] = list(_statistics_fields(opts['statistics_fields']))
    if opts.get('statistics_after') is not None:
        input_dict['options']['statistics_after'] = _statistics_stride(opts['statistics_after'], 'statistics_after', low=0)


def _own_regions(input_dict, opts, base_dir):
    """`options.regions: N` (the stride; 0 or absent: off) and `options.region_list: [{field: rho, below: 850.0, name: cavitated},
    ...]` (_region_entries)."""
    grid = input_dict.get('grid') or {}
    if opts.get('regions') is not None:
        input_dict['options']['regions'] = _regions_stride(opts['regions'], allow_zero=True)
    if opts.get('region_list') is not None:
        input_dict['options']['region_list'] = _region_entries(opts['region_list'], int(grid['Nx']) if 'Nx' in grid else None,
                                                               int(grid['Ny']) if 'Ny' in grid else None, where='options.region_list')
    if input_dict['options'].get('regions') and not input_dict['options'].get('region_list'):
        raise ValueError("options.regions: options.region_list must list the regions")


def _own_lines(input_dict, opts, base_dir):
    """`options.lines: N` (the stride; 0 or absent: off) and `options.line_list: [{along: x}, {along: y, at: [1, 32], name: band}]`
    (_line_entries)."""
    grid = input_dict.get('grid') or {}
    if opts.get('lines') is not None:
        input_dict['options']['lines'] = _lines_stride(opts['lines'], allow_zero=True)
    if opts.get('line_list') is not None:
        input_dict['options']['line_list'] = _line_entries(opts['line_list'], int(grid['Nx']) if 'Nx' in grid else None,
                                                           int(grid['Ny']) if 'Ny' in grid else None, where='options.line_list')
    if input_dict['options'].get('lines') and not input_dict['options'].get('line_list'):
        raise ValueError("options.lines: options.line_list must list the lines")


def _own_frames(input_dict, opts, base_dir):
    """`options.frames: N` (the stride; 0 or absent: off) and `options.frame_spec: {fields: [rho, p], window: [ix0, ix1, iy0, iy1],
    stride: [sx, sy], reduce: mean, dtype: f4, capacity: n}` (_frame_spec; the window is checked against the grid, when the input
    has one)."""
    grid = input_dict.get('grid') or {}
    if opts.get('frames') is not None:
        input_dict['options']['frames'] = _frames_stride(opts['frames'], allow_zero=True)
    if opts.get('frame_spec') is not None:
        spec = _frame_spec(opts['frame_spec'], int(grid['Nx']) if 'Nx' in grid else None, int(grid['Ny']) if 'Ny' in grid else None,
                           where='options.frame_spec')
        input_dict['options']['frame_spec'] = dict(spec, fields=list(spec['fields']))


def _own_init_from(input_dict, opts, base_dir):
    """`options.init_from: path` (a checkpoint to start from, Problem.init_from).  A relative path is relative to the YAML file
    (`base_dir`; a string has none: the working directory)."""
    path = opts.get('init_from')
    if path is None:
        return
    if not isinstance(path, str) or not path:
        raise ValueError(f"options.init_from: the path of a checkpoint file is required, got {path!r}")
    input_dict['options']['init_from'] = os.path.normpath(os.path.join(base_dir or os.getcwd(), path))


_OWN_KEYS = (_own_checkpoint_freq, _own_probes, _own_integrals, _own_extrema, _own_elastic_series, _own_weighted, _own_statistics,
             _own_regions, _own_lines, _own_frames, _own_changes, _own_domain_series, _own_thinning_series, _own_init_from)


def _keep(keys, input_dict, ymlstring, base_dir=None):
    """Parse the YAML text once and apply `keys` to its `options`; nothing where the input has no options section to set them
    beside, or the text's is no mapping."""
    import yaml
    opts = (yaml.full_load(ymlstring) or {}).get('options') or {}
    if input_dict.get('options') is None or not isinstance(opts, dict):
        return
    for key in keys:
        key(input_dict, opts, base_dir)


def _keep_own_options(input_dict, ymlstring, base_dir=None):
    """All of this project's own keys, in one pass over the text (Problem.from_string, SlabProblem.from_string)."""
    _keep(_OWN_KEYS, input_dict, ymlstring, base_dir)


# one key family at a time
def _keep_checkpoint_freq(input_dict, ymlstring): _keep([_own_checkpoint_freq], input_dict, ymlstring)
def _keep_probes(input_dict, ymlstring): _keep([_own_probes], input_dict, ymlstring)
def _keep_integrals(input_dict, ymlstring): _keep([_own_integrals], input_dict, ymlstring)
def _keep_extrema(input_dict, ymlstring): _keep([_own_extrema], input_dict, ymlstring)
def _keep_elastic_series(input_dict, ymlstring): _keep([_own_elastic_series], input_dict, ymlstring)
def _keep_weighted(input_dict, ymlstring, base_dir=None): _keep([_own_weighted], input_dict, ymlstring, base_dir)
def _keep_statistics(input_dict, ymlstring): _keep([_own_statistics], input_dict, ymlstring)
def _keep_regions(input_dict, ymlstring): _keep([_own_regions], input_dict, ymlstring)
def _keep_lines(input_dict, ymlstring): _keep([_own_lines], input_dict, ymlstring)
def _keep_frames(input_dict, ymlstring): _keep([_own_frames], input_dict, ymlstring)
def _keep_changes(input_dict, ymlstring): _keep([_own_changes], input_dict, ymlstring)
def _keep_thinning_series(input_dict, ymlstring): _keep([_own_thinning_series], input_dict, ymlstring)
def _keep_domain_series(input_dict, ymlstring): _keep([_own_domain_series], input_dict, ymlstring)
def _keep_init_from(input_dict, ymlstring, base_dir=None): _keep([_own_init_from], input_dict, ymlstring, base_dir)


def _in_main_thread():
    import threading
    return threading.current_thread() is threading.main_thread()
