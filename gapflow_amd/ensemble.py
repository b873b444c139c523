"""Ensembles: many small problems advanced together, one workgroup of one launch per member (no reference counterpart:
the reference runs a parameter study -- three eccentricities of the Sommerfeld test, a Stribeck curve over U -- as one
process per problem).  DESIGN.md 3.2c.

    ens = Ensemble.sweep("journal1d.yaml", {'geometry.eps': [0.5, 0.7, 0.9], 'geometry.U': [0.05, 0.1]})
    ens.set_integrals(every=10)                 # load, friction and flow histories, recorded inside the launches
    ens.set_extrema(every=10)                   # peak pressure, minimum film, ... with their cells, likewise
    ens.set_probes([[50, 1]])                   # rho, jx, jy, p at a cell after every step, likewise
    ens.run()
    loads = [r['load'] for r in ens.film_integrals()]
    history = [s.load for s in ens.integrals]
    peaks = [s.p_max for s in ens.extrema]

An ensemble HOLDS its `Problem` objects, it does not copy them: after `run()` or `step()` every member is, bit for bit, what
the same call on it alone would have made it (`q`, `step`, `simtime`, `dt`, `residual`, `residual_buffer`, `history`, derived
fields, output files), and it can go on alone.  Members may differ in everything -- grid, gap, edges, equation of state,
step size, stop condition -- but each must fit one of the two one-workgroup kernels; what does not is refused when the
ensemble is built, by name and with the reason.

Two tiers (`Ensemble.tiers`, `member_tier`): 'lds' -- up to 1200 cells, ghost cells included, the planes in LDS
(csrc/small_kernel.hip); such a member is bit for bit its solo run.  'workspace' -- up to 16384 cells (126 x 126 interior
cells: the reference's 2-D set-ups), the planes in a workspace in device memory that the ensemble owns (csrc/mid_kernel.hip);
such a member is bit for bit the same whoever else is in the ensemble and however its steps are split into calls, and agrees
with its solo run (another kernel) to rounding.
"""
import ctypes as C
import itertools
import os
import signal
from collections import namedtuple
from datetime import datetime

import numpy as np

from . import _lib
from .problem import (Problem, _extrema_series, _film_series, _in_main_thread, _probe_series, _save_extrema_series, _save_film_series,
                      _save_probe_series, _termination_signals)
from .series import ALL_SERIES, _Series, _extrema_stride, _integral_sections, _integral_stride, _probe_cells


# The ensemble's series, in the order _advance collects them and run() writes them, as series.ALL_SERIES lists a Problem's.
# marker: the Ensemble attribute that is None while the series is off (its set_* sets it, and the per-member _Series list);
# clear: the library's entry point that disarms it; collect(i, entries, before), view(i): Ensemble's methods -- member i's records
# of a call to its _Series, its series as the named tuple Problem gives; save(outdir, view): the file a solo run writes.
_Row = namedtuple('_Row', 'marker clear collect view save')
ENSEMBLE_SERIES = {
    'integrals': _Row('_integral_every', 'gpf_ensemble_integrals_clear', '_collect_integrals', '_member_integrals', _save_film_series),
    'extrema': _Row('_extrema_every', 'gpf_ensemble_extrema_clear', '_collect_extrema', '_member_extrema', _save_extrema_series),
    'probes': _Row('_probe_cells', 'gpf_ensemble_probes_clear', '_collect_probes', '_member_probes', _save_probe_series),
}


def member_tier(nx, ny):
    """The tier an Nx x Ny member gets: 'lds', 'workspace', or None for a grid no tier takes.  Host only."""
    cells = (int(nx) + 2) * (int(ny) + 2)
    if cells * _lib.SMALL_GRID_DOUBLES_PER_CELL * 8 <= _lib.SMALL_GRID_LDS_BYTES:
        return 'lds'
    return 'workspace' if cells <= _lib.MID_GRID_MAX_CELLS else None


def workspace_bytes(nx, ny):
    """Bytes of device memory an Nx x Ny member's workspace takes: MID_GRID_DOUBLES_PER_CELL doubles per cell, ghost cells
    included, rounded up to 256 (csrc/mid_layout.hpp).  Host only."""
    raw = (int(nx) + 2) * (int(ny) + 2) * _lib.MID_GRID_DOUBLES_PER_CELL * 8
    return (raw + 255) // 256 * 256


def _refusal(p):
    """Why Problem `p` cannot be a member, as (exception class, reason), or None.  Host only: mirrors gpf_ensemble_create."""
    if os.environ.get('GPF_SMALL_GRID') is not None and _atoi(os.environ['GPF_SMALL_GRID']) == 0:
        return NotImplementedError, "GPF_SMALL_GRID=0 turns the one-workgroup kernel off, and an ensemble is made of nothing else"
    if p._gp_models or p.has_gp_model:
        return NotImplementedError, "surrogate (GP) closures step stage-wise, with the host between the stages"
    if p._cfg.thinning:
        return NotImplementedError, "shear thinning steps stage-wise (it needs grad p)"
    if p._elastic or p.topo.elastic:
        return NotImplementedError, "an elastic gap steps stage-wise and deforms between steps"
    if member_tier(p._shape[0] - 2, p._shape[1] - 2) is None:
        return NotImplementedError, (f"its {p.grid['Nx']} x {p.grid['Ny']} grid does not fit one workgroup's LDS "
                                     f"({_lib.SMALL_GRID_DOUBLES_PER_CELL} doubles per cell, ghost cells included, in "
                                     f"{_lib.SMALL_GRID_LDS_BYTES // 1024} KB) nor the workspace tier (at most "
                                     f"{_lib.MID_GRID_MAX_CELLS} cells, ghost cells included)")
    for row in sorted((r for r in ALL_SERIES if r.refusal), key=lambda r: r.refusal[0]):
        if getattr(p, row.marker, None) is not None:            # (getattr: a Problem made without __init__ may lack the attribute)
            return NotImplementedError, f"{row.noun} are armed on it ({row.refusal[1]}): {row.clear}(), or run it alone"
    return None


def _atoi(text):
    """C's atoi, which the library applies to GPF_SMALL_GRID: leading blanks, a sign, digits; 0 where there are none."""
    import re
    m = re.match(r'\s*([+-]?\d+)', text)
    return int(m.group(1)) if m else 0


def sweep_members(base, axes):
    """The members of a sweep over `axes` = {'section.key': [values...]} of the YAML dictionary `base`: one dictionary per
    element of the Cartesian product, with the FIRST axis slowest and the last fastest (itertools.product over the axes in the
    order given), and beside them the list of {dotted key: value} each one got.  KeyError for a section or key that `base`
    does not hold (a sweep varies what the input states, it adds nothing).  Host only."""
    import copy
    if not axes:
        raise ValueError("sweep: at least one 'section.key': [values] axis is required")
    names = list(axes)
    for name in names:
        parts = str(name).split('.')
        if len(parts) < 2:
            raise KeyError(f"sweep: '{name}' is not of the form section.key")
        node = base
        for k, part in enumerate(parts):
            if not isinstance(node, dict) or part not in node:
                what = 'section' if k == 0 else 'key'
                raise KeyError(f"sweep: the input has no {what} '{part}' (axis '{name}')")
            node = node[part]
        values = axes[name]
        if isinstance(values, (str, bytes, dict)) or not hasattr(values, '__len__') or len(values) < 1:
            raise ValueError(f"sweep: axis '{name}' needs a non-empty list of values, got {values!r}")
    dicts, params = [], []
    for combo in itertools.product(*[list(axes[name]) for name in names]):
        d = copy.deepcopy(base)
        for name, v in zip(names, combo):
            parts = name.split('.')
            node = d
            for part in parts[:-1]:
                node = node[part]
            node[parts[-1]] = v.item() if isinstance(v, np.generic) else v
        dicts.append(d)
        params.append(dict(zip(names, combo)))
    return dicts, params


class Ensemble:
    """`Ensemble(problems, tier='auto')`: the given `Problem` objects, advanced together.  tier='workspace' gives every member
    the workspace tier, those that fit LDS too.  See the module's text."""

    def __init__(self, problems, tier='auto'):
        if tier not in ('auto', 'workspace'):
            raise ValueError(f"Ensemble: tier = {tier!r}, 'auto' or 'workspace' required")
        problems = list(problems)
        if len(problems) < 1:
            raise ValueError("Ensemble: at least one member is required (an empty list was given)")
        for i, p in enumerate(problems):
            if not isinstance(p, Problem):
                raise TypeError(f"Ensemble: member {i} is a {type(p).__name__}, not a Problem")
            for j in range(i):
                if problems[j] is p:
                    raise ValueError(f"Ensemble: member {i} is the same Problem as member {j} (two workgroups would write the same buffers)")
            why = _refusal(p)
            if why is not None:
                raise why[0](f"Ensemble: member {i}: {why[1]}")
            if p._cfg.device != problems[0]._cfg.device:
                raise ValueError(f"Ensemble: member {i} lives on device {p._cfg.device}, member 0 on device {problems[0]._cfg.device} "
                                 "(one launch needs one device)")
        self.problems = problems
        self.parameters = None              # sweep(): what each member got, {dotted key: value}
        self._integral_every = None         # set_integrals: the stride, per member its sections and its series
        self._extrema_every = None          # set_extrema: the stride, per member its series
        self._probe_cells = None            # set_probes: per member its cells and its series
        self._lib = problems[0]._lib
        self._e = C.c_void_p()
        handles = (C.c_void_p * len(problems))(*[p._h.value for p in problems])
        flags = _lib.ENSEMBLE_FORCE_WORKSPACE if tier == 'workspace' else 0
        _lib.check(self._lib.gpf_ensemble_create2(handles, len(problems), flags, C.byref(self._e)))

    def __del__(self):
        e = getattr(self, '_e', None)
        if e is not None and e.value:
            self._lib.gpf_ensemble_destroy(e)
            e.value = None

    def __len__(self):
        return len(self.problems)

    def __getitem__(self, i):
        return self.problems[i]

    def __iter__(self):
        return iter(self.problems)

    # -------------------------------------------------------------------------------------
    # constructors
    # -------------------------------------------------------------------------------------
    @classmethod
    def from_yaml(cls, fnames, device=0):
        """One member per input file, in the order given."""
        return cls([Problem.from_yaml(f, device=device) for f in fnames])

    @classmethod
    def sweep(cls, yaml_path_or_string, axes, device=0):
        """One member per element of the Cartesian product of `axes` = {'section.key': [values...]} over the input: dotted keys
        address the YAML sections ('geometry.eps', 'numerics.tol', 'properties.piezo.aB').  Order: itertools.product over the
        axes as given -- the first axis varies slowest, the last fastest; `parameters[m]` holds what member m got.  A section or
        key the input does not hold raises KeyError before any problem is built.  A non-silent input with a fixed output
        directory would have every member write into the same one: sweep 'options.output' too, or keep `use_tstamp`."""
        import yaml
        text = yaml_path_or_string if isinstance(yaml_path_or_string, str) else os.fspath(yaml_path_or_string)
        if '\n' not in text and os.path.exists(text):
            with open(text, 'r') as f:
                text = f.read()
        base = yaml.full_load(text)
        if not isinstance(base, dict):
            raise ValueError("sweep: the input is not a YAML mapping of sections")
        dicts, params = sweep_members(base, axes)
        ens = cls([Problem.from_string(yaml.safe_dump(d), device=device) for d in dicts])
        ens.parameters = params
        return ens

    # -------------------------------------------------------------------------------------
    # stepping
    # -------------------------------------------------------------------------------------
    def _advance(self, counts, honor_stop):
        """counts[m] steps for member m (0: leave it alone) in one library call; returns the per-step records per member."""
        ps = self.problems
        for i, (p, n) in enumerate(zip(ps, counts)):
            if n < 0 or n > _lib.LOG_CAPACITY:
                raise ValueError(f"Ensemble: member {i}: {n} steps, 0 .. {_lib.LOG_CAPACITY} (the device log's capacity) per call required")
            if n == 0:
                continue
            if p.step is None:
                raise RuntimeError(f"Ensemble: member {i}: call _pre_run() (or run()) before step()")
            why = _refusal(p)
            if why is not None:
                raise why[0](f"Ensemble: member {i}: {why[1]}")
        for p, n in zip(ps, counts):
            if n:
                p._sync_to_device()
        arr = (C.c_int64 * len(ps))(*[int(n) for n in counts])
        nexec = (C.c_int64 * len(ps))()
        _lib.check(self._lib.gpf_ensemble_step(self._e, arr, int(honor_stop), nexec))
        out, armed = [], self._armed()
        for i, (p, n) in enumerate(zip(ps, counts)):
            if n == 0:
                out.append([])
                continue
            log = (_lib.GpfScalars * n)()
            _lib.check(self._lib.gpf_ensemble_log(self._e, i, log, n, None))
            before = p.step
            out.append(p._absorb_batch(log, n, int(nexec[i]) - before, before))
            for row in armed:
                getattr(self, row.collect)(i, out[-1], before)
        return out

    def step(self, n):
        """Advance every member by n steps -- an int, or one count per member (0 leaves a member alone) -- as `Problem.update()`
        would, n times: no stop at convergence or max_it."""
        counts = [int(n)] * len(self.problems) if isinstance(n, (int, np.integer)) else [int(k) for k in n]
        if len(counts) != len(self.problems):
            raise ValueError(f"Ensemble.step: {len(counts)} counts for {len(self.problems)} members")
        todo = list(counts)
        while any(todo):                # the device log holds 4096 records per member and call
            now = [min(k, _lib.LOG_CAPACITY) for k in todo]
            self._advance(now, honor_stop=False)
            todo = [k - d for k, d in zip(todo, now)]

    def _receive_signal(self, signum, frame):
        if signum in _termination_signals():
            for p in self.problems:
                p._stop = True

    def run(self, keep_open=False):
        """For every member what `Problem.run()` does for it alone: `_pre_run` where needed, batches whose length per member
        follows the rule of `Problem.run` (its own write_freq, max_it, checkpoint_freq; 4096), frames and checkpoints at its own
        multiples, `_post_run` when IT ends.  A member that has converged, reached max_it or been rolled back takes no further
        part.  A termination signal stops all members."""
        ps = self.problems
        cfs = [p._run_begin() for p in ps]
        old = {s: signal.signal(s, self._receive_signal) for s in _termination_signals()} if _in_main_thread() else {}
        tic = datetime.now()
        for p in ps:
            p._tic = tic
        running = [True] * len(ps)

        def retire():
            for i, p in enumerate(ps):
                if running[i] and not p._run_active():
                    running[i] = False
                    p._run_end(cfs[i], keep_open)
                    if keep_open or p.options['silent']:
                        continue
                    for row in self._armed():            # the arrays a solo run's integrals.npz / extrema.npz / probes.npz hold
                        row.save(p.outdir, getattr(self, row.view)(i))

        try:
            retire()
            while any(running):
                counts = [p._run_batch_length(cf) if on else 0 for p, cf, on in zip(ps, cfs, running)]
                self._advance(counts, honor_stop=True)
                for p, cf, on in zip(ps, cfs, running):
                    if on:
                        p._run_after_batch(cf)
                retire()
        finally:
            for s, hdl in old.items():
                signal.signal(s, hdl)

    # -------------------------------------------------------------------------------------
    # the series (ENSEMBLE_SERIES above): what they share
    # -------------------------------------------------------------------------------------
    def _armed(self):
        """The rows of the series that are armed: the only ones whose collect and view may be called."""
        return [row for row in ENSEMBLE_SERIES.values() if getattr(self, row.marker) is not None]

    def _clear(self, row):
        if getattr(self, row.marker) is not None:
            _lib.check(getattr(self._lib, row.clear)(self._e))
        setattr(self, row.marker, None)

    def _views(self, row):
        if getattr(self, row.marker) is None:
            return None
        return [getattr(self, row.view)(i) for i in range(len(self.problems))]

    # -------------------------------------------------------------------------------------
    # film-integral series
    # -------------------------------------------------------------------------------------
    def set_integrals(self, every=1, sections_x=None, sections_y=None):
        """Record `Problem.set_integrals`' record for EVERY member after each of its committed steps whose count is a multiple
        of `every`, inside the ensemble's launches: both one-workgroup kernels write it after the step's commit, bit for bit what
        `film_integrals()` gives for the same state, and no launch is cut.  sections_x / sections_y: None for each member's first
        and last interior row / column; a list holds for all members and must lie inside every member's interior (ValueError
        naming the member otherwise).  Starts new series (see ``integrals``).  A member that has `set_integrals` armed on itself
        is still refused; the members' own `integrals` stay None."""
        every = _integral_stride(every)
        layout = []
        for i, p in enumerate(self.problems):
            try:
                layout.append((_integral_sections(sections_x, p.grid['Nx'], 'sections_x'), _integral_sections(sections_y, p.grid['Ny'], 'sections_y')))
            except ValueError as err:
                raise ValueError(f"Ensemble.set_integrals: member {i}: {err}") from None
        i32p = C.POINTER(C.c_int32)
        ax = np.array(sections_x if sections_x is not None else [], dtype=np.int32)
        ay = np.array(sections_y if sections_y is not None else [], dtype=np.int32)
        _lib.check(self._lib.gpf_ensemble_integrals_set(self._e, every, len(ax), ax.ctypes.data_as(i32p) if len(ax) else None,
                                                        len(ay), ay.ctypes.data_as(i32p) if len(ay) else None))
        self._integral_every, self._integral_sections = every, layout
        self._integral_series = [_Series(f'Ensemble integrals: member {i}', every) for i in range(len(self.problems))]

    def clear_integrals(self):
        """Stop recording and drop the series."""
        self._clear(ENSEMBLE_SERIES['integrals'])

    def _collect_integrals(self, i, entries, before):
        """Member i's records of the call that took its step count from `before` through `entries` (its committed steps).
        Only while the series is armed (_advance calls it through _armed())."""
        sx, sy = self._integral_sections[i]

        def read(b, n, steps, have):
            _lib.check(self._lib.gpf_ensemble_integrals_read(self._e, i, _lib.as_dp(b[0]), n, steps, have))
        self._integral_series[i].collect(read, entries, before, [((len(_lib.INTEGRAL_SUMS) + len(sx) + len(sy),), np.float64)])

    def _member_integrals(self, i):
        return _film_series(self._integral_series[i], *self._integral_sections[i])

    @property
    def integrals(self):
        """One FilmIntegrals(step, time, load, ..., flow_x, flow_y, sections_x, sections_y) per member -- `Problem.integrals`'
        type -- of every recorded step since set_integrals, across `step()` and `run()` calls; None when none are armed."""
        return self._views(ENSEMBLE_SERIES['integrals'])

    # -------------------------------------------------------------------------------------
    # extrema series and point probes
    # -------------------------------------------------------------------------------------
    def set_extrema(self, every=1):
        """Record `Problem.set_extrema`'s record -- p_max, p_min, rho_max, rho_min, h_min, u_max, v_max, each with its cell -- for
        EVERY member after each of its committed steps whose count is a multiple of `every`, inside the ensemble's launches: both
        one-workgroup kernels write it after the step's commit, bit for bit what `field_extrema()` gives for the same state, and
        no launch is cut.  Starts new series (see ``extrema``).  A member that has `set_extrema` armed on itself is still
        refused; the members' own `extrema` stay None."""
        every = _extrema_stride(every, allow_zero=False)
        _lib.check(self._lib.gpf_ensemble_extrema_set(self._e, every))
        self._extrema_every = every
        self._extrema_series = [_Series(f'Ensemble extrema: member {i}', every) for i in range(len(self.problems))]

    def clear_extrema(self):
        """Stop recording and drop the series."""
        self._clear(ENSEMBLE_SERIES['extrema'])

    def _collect_extrema(self, i, entries, before):
        """Member i's records of the call that took its step count from `before` through `entries` (its committed steps).
        Only while the series is armed (_advance calls it through _armed())."""
        nq = len(_lib.EXTREMA_NAMES)

        def read(b, n, steps, have):
            _lib.check(self._lib.gpf_ensemble_extrema_read(self._e, i, _lib.as_dp(b[0]), b[1].ctypes.data_as(C.POINTER(C.c_int32)), n, steps, have))
        self._extrema_series[i].collect(read, entries, before, [((nq,), np.float64), ((nq, 2), np.int32)])

    def _member_extrema(self, i):
        return _extrema_series(self._extrema_series[i])

    @property
    def extrema(self):
        """One FieldExtrema(step, time, p_max, ..., v_max, cells, index) per member -- `Problem.extrema`'s type -- of every recorded
        step since set_extrema, across `step()` and `run()` calls; None when none are armed."""
        return self._views(ENSEMBLE_SERIES['extrema'])

    def set_probes(self, cells, pressure=True):
        """Record `Problem.set_probes`' record -- rho, jx, jy (and p) at `cells` -- for EVERY member after each of its committed
        steps, inside the ensemble's launches.  cells: one list of [ix, iy] pairs of the ghosted index space that holds for all
        members, or one such list per member (a list of len(ensemble) lists); every cell must lie inside its member's ghosted grid
        (ValueError naming the member otherwise).  The records of one call live in one device buffer, 4096 x cells x values
        doubles per member; beyond 256 MiB (GPF_ENSEMBLE_PROBES_MB sets another limit, in MiB) the library refuses.  Starts new
        series (see ``probes``).  A member that has `set_probes` armed on itself is still refused; the members' own `probes` stay
        None."""
        ps = self.problems

        def is_pair(c):
            return not isinstance(c, (str, bytes, dict)) and hasattr(c, '__len__') and len(c) == 2 and not any(hasattr(v, '__len__') for v in c)
        per_member = not isinstance(cells, (str, bytes, dict)) and hasattr(cells, '__len__') and len(cells) > 0 and \
            all(not isinstance(c, (str, bytes, dict)) and hasattr(c, '__len__') and not is_pair(c) for c in cells)
        if per_member and len(cells) != len(ps):
            raise ValueError(f"Ensemble.set_probes: {len(cells)} lists of cells for {len(ps)} members (one list for all, or one per member)")
        checked = []
        for i, p in enumerate(ps):
            try:
                checked.append(_probe_cells(cells[i] if per_member else cells, p._shape))
            except ValueError as err:
                raise ValueError(f"Ensemble.set_probes: member {i}: {err}") from None
        i32p = C.POINTER(C.c_int32)
        counts = np.array([len(c) for c in checked] if per_member else [len(checked[0])], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate(checked) if per_member else checked[0], dtype=np.int32)
        _lib.check(self._lib.gpf_ensemble_probes_set(self._e, int(per_member), counts.ctypes.data_as(i32p), flat.ctypes.data_as(i32p), int(bool(pressure))))
        self._probe_cells, self._probe_pressure = checked, bool(pressure)
        self._probe_series = [_Series(f'Ensemble probes: member {i}') for i in range(len(ps))]

    def clear_probes(self):
        """Stop recording and drop the series."""
        self._clear(ENSEMBLE_SERIES['probes'])

    def _collect_probes(self, i, entries, before=None):
        """Member i's probe records of the call that returned `entries` (its committed steps' scalar records).  Only while
        probes are set (_advance calls it through _armed())."""

        def read(out, n, first, have):
            _lib.check(self._lib.gpf_ensemble_probes_read(self._e, i, _lib.as_dp(out), n, first, have))
        self._probe_series[i].collect_every_step(read, entries, (len(self._probe_cells[i]), 4 if self._probe_pressure else 3))

    def _member_probes(self, i):
        return _probe_series(self._probe_series[i], self._probe_cells[i], self._probe_pressure)

    @property
    def probes(self):
        """One ProbeSeries(step, time, cells, rho, jx, jy, p) per member -- `Problem.probes`' type -- of every step committed
        since set_probes, across `step()` and `run()` calls; None when no probes are set."""
        return self._views(ENSEMBLE_SERIES['probes'])

    # -------------------------------------------------------------------------------------
    # views
    # -------------------------------------------------------------------------------------
    @property
    def tiers(self):
        """The tier of every member as the library assigned it: 'lds' or 'workspace'."""
        out = []
        for i in range(len(self.problems)):
            t = C.c_int32(0)
            _lib.check(self._lib.gpf_ensemble_member_info(self._e, i, C.byref(t), None))
            out.append(_lib.ENSEMBLE_TIERS[t.value])
        return out

    @property
    def steps(self):
        """Step count of every member (-1 before its `_pre_run`)."""
        return np.array([-1 if p.step is None else p.step for p in self.problems], dtype=np.int64)

    @property
    def converged(self):
        """`Problem.converged` of every member (False before its `_pre_run`)."""
        return np.array([p.step is not None and p.converged for p in self.problems], dtype=bool)

    def film_integrals(self):
        """`Problem.film_integrals()` of every member's current state: load, friction and flow rates -- what a sweep is usually for."""
        return [p.film_integrals() for p in self.problems]

    def field_extrema(self):
        """`Problem.field_extrema()` of every member's current state: peak pressure, lowest density, smallest gap, largest
        velocity components, each with its cell."""
        return [p.field_extrema() for p in self.problems]
