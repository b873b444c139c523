"""Host side of the recorded series: the one recorder, `_Series`; the one table of the series' lifecycle,
`SERIES`; the one stride check; and the validators of what the `set_*` methods and the YAML keys are given.  Nothing here
touches a device, and nothing here imports `problem`: a new series is one row of `SERIES_MORE` (Problem and Ensemble walk
`ALL_SERIES`), one `_Series` in its `set_*` and a two-line `read` closure in its `_collect_*`.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib

_I64P = C.POINTER(C.c_int64)


def _integral_records(base, ran, every):
    """Records a stepping call leaves that took the step count from `base` over `ran` committed steps at stride `every`: the
    multiples of `every` in (base, base + ran].  The slot of the step that takes the count to `expect` is
    _integral_records(base, expect - base, every) - 1 (csrc/api_series.inc: series_count)."""
    return (base + ran) // every - base // every if ran > 0 else 0


class _Series:
    """One series as the host keeps it: `steps`, `times` and, per stepping call that left records, one block -- a tuple of the
    arrays its read call filled (regions, extrema and the elastic series read two buffers per call, the others one)."""

    def __init__(self, label, every=1):
        self.label, self.every = label, every
        self.reset()

    def reset(self):
        self.steps, self.times, self.blocks = [], [], []

    def collect(self, read, entries, before, shapes):
        """Append the records of the stepping call that took the step count from `before` through `entries` (its committed
        steps' scalar records).  shapes: per buffer, (trailing shape, dtype); read(buffers, n, steps_ptr, have_ref) makes the
        library's read call for n records.  GapflowHipError, and nothing appended, unless the library hands out exactly the
        multiples of the stride among the committed steps."""
        if not entries:
            return
        ran, every = len(entries), self.every
        n = _integral_records(before, ran, every)
        buffers = tuple(np.zeros((n,) + tuple(shape), dtype=dtype) for shape, dtype in shapes)
        steps = np.zeros(n, dtype=np.int64)
        have = C.c_int64(0)
        read(buffers, n, steps.ctypes.data_as(_I64P), C.pointer(have))
        want = [s for s in range(before + 1, before + ran + 1) if s % every == 0]
        if have.value != n or steps.tolist() != want:
            raise _lib.GapflowHipError(f"{self.label}: {have.value} records of steps {steps.tolist()} for the committed steps "
                                       f"{before + 1}..{before + ran} at stride {every}")
        self.steps.extend(want)
        self.times.extend(entries[s - before - 1].simtime for s in want)
        self.blocks.append(buffers)

    def collect_every_step(self, read, entries, shape):
        """The same for a series that records every committed step into one float64 buffer (the probes): the library names the
        first step and the count, read(buffer, n, first_ref, have_ref)."""
        if not entries:
            return
        out = np.zeros((len(entries),) + tuple(shape))
        first, have = C.c_int64(0), C.c_int64(0)
        read(out, len(entries), C.pointer(first), C.pointer(have))
        if have.value != len(entries) or first.value != entries[0].step:
            raise _lib.GapflowHipError(f"{self.label}: {have.value} records from step {first.value} for {len(entries)} committed steps "
                                       f"from step {entries[0].step}")
        self.steps.extend(int(e.step) for e in entries)
        self.times.extend(e.simtime for e in entries)
        self.blocks.append((out,))

    def stacked(self, k, shape, dtype=np.float64):
        """Buffer k of every block, concatenated along the records; (0,) + shape of `dtype` while there are none."""
        return np.concatenate([b[k] for b in self.blocks]) if self.blocks else np.empty((0,) + tuple(shape), dtype=dtype)

    def step_array(self):
        return np.array(self.steps, dtype=np.int64)

    def time_array(self):
        return np.array(self.times, dtype=np.float64)


# The series' lifecycle, in the order Problem arms, collects and writes them.  marker: the Problem attribute that is None while
# the series is off; recorder: the attribute of its _Series (None: no host-side records); collect, write: Problem's methods;
# noun, clear: what Ensemble's refusal says; refusal: (rank among Ensemble's checks, reason), None where an earlier check
# covers it; fused: whether the fused batch path collects it (the elastic series exists on the stage-wise path only).
_Row = namedtuple('_Row', 'marker recorder collect write noun clear refusal fused')
CUTS, SLOTS = "they cut the batch per member", "their records need per-member slots"
SERIES = (
    _Row('_probe_cells', '_probe_rec', '_collect_probes', '_write_probes', 'probes', 'clear_probes', (5, SLOTS), True),
    _Row('_integral_every', '_integral_rec', '_collect_integrals', '_write_integrals', 'film integrals', 'clear_integrals', (0, CUTS), True),
    _Row('_weighted_every', '_weighted_rec', '_collect_weighted', '_write_weighted', 'weighted integrals', 'clear_weighted_integrals', (1, CUTS), True),
    _Row('_regions_every', '_regions_rec', '_collect_regions', '_write_regions', 'regions', 'clear_regions', (3, CUTS), True),
    _Row('_lines_every', '_lines_rec', '_collect_lines', '_write_lines', 'lines', 'clear_lines', (4, CUTS), True),
    _Row('_extrema_every', '_extrema_rec', '_collect_extrema', '_write_extrema', 'extrema', 'clear_extrema', (6, SLOTS), True),
    _Row('_elastic_series_every', '_elastic_series_rec', '_collect_elastic_series', '_write_elastic_series', 'elastic series',
         'clear_elastic_series', None, False),
    _Row('_stats_every', None, None, '_write_statistics', 'statistics', 'clear_statistics', (2, CUTS), False),
)
# The series added since: behind SERIES in the arming, collecting, writing and refusal order
SERIES_MORE = (
    _Row('_frames_every', '_frames_rec', '_collect_frames', '_write_frames', 'frames', 'clear_frames', (8, CUTS), True),
    _Row('_changes_every', '_changes_rec', '_collect_changes', '_write_changes', 'changes', 'clear_changes', (7, CUTS), True),
)
ALL_SERIES = SERIES + SERIES_MORE
# The series that exist on the stage-wise path alone and were added since (the elastic series is the one in SERIES): never
# collected by a fused batch, never an Ensemble's concern (it refuses such a problem before it looks at its series).  Problem's
# _pre_run and _post_run walk them behind ALL_SERIES.
SERIES_STAGEWISE = (
    _Row('_thinning_series_every', '_thinning_series_rec', '_collect_thinning_series', '_write_thinning_series', 'thinning series',
         'clear_thinning_series', None, False),
)


def _stride(label, value, low, what='the stride'):
    """`value` as an int; ValueError unless it is an integer (no bool) >= low."""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or value < low:
        raise ValueError(f"{label}: {what} must be an integer >= {low}, got {value!r}")
    return int(value)


def _integral_stride(every): return _stride('integrals', every, 1)
def _weighted_stride(every, allow_zero=False): return _stride('weighted integrals', every, 0 if allow_zero else 1)
def _regions_stride(every, allow_zero=False): return _stride('regions', every, 0 if allow_zero else 1)
def _lines_stride(every, allow_zero=False): return _stride('lines', every, 0 if allow_zero else 1)
def _extrema_stride(every, allow_zero=True): return _stride('extrema', every, 0 if allow_zero else 1)
def _elastic_series_stride(every, allow_zero=True): return _stride('elastic series', every, 0 if allow_zero else 1)
def _thinning_series_stride(every, allow_zero=True): return _stride('thinning series', every, 0 if allow_zero else 1)
def _changes_stride(every, allow_zero=True): return _stride('changes', every, 0 if allow_zero else 1)
def _frames_stride(every, allow_zero=False): return _stride('frames', every, 0 if allow_zero else 1)
def _statistics_stride(v, key, low): return _stride('statistics', v, low, key)


def _probe_cells(cells, shape=None):
    """Probe cells as an (n, 2) integer array; ValueError for anything that is not 1..256 pairs of integers or, when the ghosted
    shape (Nx+2, Ny+2) is given, for a cell outside it.  Host only: no library call."""
    if isinstance(cells, (str, bytes, dict)) or not hasattr(cells, '__len__'):
        raise ValueError(f"probes: a list of [ix, iy] cells is required, got {cells!r}")
    if len(cells) < 1:
        raise ValueError("probes: at least one cell is required (clear_probes removes them)")
    if len(cells) > _lib.PROBE_MAX:
        raise ValueError(f"probes: {len(cells)} cells, at most {_lib.PROBE_MAX} per problem")
    out = np.empty((len(cells), 2), dtype=np.int64)
    for k, c in enumerate(cells):
        ok = not isinstance(c, (str, bytes, dict)) and hasattr(c, '__len__') and len(c) == 2 and \
            all(isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) for v in c)
        if not ok:
            raise ValueError(f"probes: entry {k} must be a pair of integers [ix, iy], got {c!r}")
        ix, iy = int(c[0]), int(c[1])
        if shape is not None and not (0 <= ix < shape[0] and 0 <= iy < shape[1]):
            raise ValueError(f"probes: cell ({ix}, {iy}) (entry {k}) lies outside the ghosted grid 0..{shape[0] - 1} x 0..{shape[1] - 1}")
        out[k] = ix, iy
    return out


def _integral_sections(sections, n, what):
    """Interior rows / columns of the flow sections as a list of ints; None: the first and last of 1..n (one where n == 1).
    ValueError for anything that is not 1..8 integers within 1..n.  Host only: no library call."""
    if sections is None:
        return [1, n] if n > 1 else [1]
    if isinstance(sections, (str, bytes, dict)) or not hasattr(sections, '__len__'):
        raise ValueError(f"integrals: {what} must be a list of interior indices, got {sections!r}")
    if not 1 <= len(sections) <= _lib.INTEGRAL_MAX_SECTIONS:
        raise ValueError(f"integrals: {what} holds {len(sections)} sections, 1 to {_lib.INTEGRAL_MAX_SECTIONS} required")
    out = []
    for k, v in enumerate(sections):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"integrals: {what}[{k}] must be an integer, got {v!r}")
        if not 1 <= int(v) <= n:
            raise ValueError(f"integrals: {what}[{k}] = {int(v)} lies outside the interior 1..{n}")
        out.append(int(v))
    return out


DOMAIN_SERIES_KEYS = ('integrals', 'extrema', 'sections_x', 'sections_y')


def _domain_series_entry(given, nx=None, ny=None, where='domain series'):
    """What SlabProblem.set_domain_series / options.domain_series is given, checked and completed: {integrals, extrema, sections_x,
    sections_y} with the two strides as ints (0 or absent: that series is off) and the sections as _integral_sections leaves them
    (None: the first and last of the domain), checked against the domain's nx, ny where given.  ValueError for an unknown key and,
    with the film integrals' and the extrema's own messages, for a bad stride or section.  Host only: no library call."""
    if not isinstance(given, dict) or set(given) - set(DOMAIN_SERIES_KEYS):
        raise ValueError(f"{where}: a mapping with the keys {list(DOMAIN_SERIES_KEYS)} is required, got {given!r}")
    out = {'integrals': _stride('integrals', 0 if given.get('integrals') is None else given['integrals'], 0),
           'extrema': _extrema_stride(0 if given.get('extrema') is None else given['extrema'])}
    for key, n in (('sections_x', nx), ('sections_y', ny)):
        s = given.get(key)
        out[key] = None if s is None else _integral_sections(s, 2**31 - 1 if n is None else int(n), key)
    return out


def _domain_chunk(base, n, strides, cap):
    """The most of `n` steps a stepping call that begins at step count `base` may take so that no series (its stride in `strides`,
    0: off) leaves more than `cap` records, _integral_records(base, ., every) <= cap: SlabProblem.advance splits a longer call
    there, and the next piece's slots start at 0 again.  At least 1 for cap >= 1."""
    for every in strides:
        if every:
            n = min(n, (base // every + cap + 1) * every - 1 - base)
    return n


def _weight_planes(weights, names, nx, ny):
    """(planes (K, nx, ny) float64, names) of what set_weighted_integrals is given; ValueError for a shape other than (K, nx, ny) /
    (nx, ny), K outside 1..8, a weight that is not finite (plane and cell named, the cell in the ghosted index space as the library
    names it) or names that do not match.  Host only: no library call."""
    try:
        a = np.array(weights, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"weighted integrals: weights must be an array of shape (K, {nx}, {ny}) or ({nx}, {ny})") from None
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[1:] != (nx, ny):
        raise ValueError(f"weighted integrals: weights of shape {np.shape(weights)}; (K, {nx}, {ny}) or ({nx}, {ny}) required "
                         "(interior cells; ghost cells never contribute)")
    if not 1 <= len(a) <= _lib.WEIGHTED_MAX_PLANES:
        raise ValueError(f"weighted integrals: {len(a)} weight planes, 1 to {_lib.WEIGHTED_MAX_PLANES} required")
    bad = np.argwhere(~np.isfinite(a))
    if len(bad):
        k, i, j = (int(v) for v in bad[0])
        raise ValueError(f"weighted integrals: weight plane {k} is not finite at cell ({i + 1}, {j + 1})")
    if names is None:
        names = [f'w{k}' for k in range(len(a))]
    if isinstance(names, (str, bytes)) or not hasattr(names, '__len__') or len(names) != len(a) or \
            not all(isinstance(n, str) and n for n in names) or len(set(names)) != len(names):
        raise ValueError(f"weighted integrals: names must be {len(a)} distinct non-empty strings, got {names!r}")
    return np.ascontiguousarray(a), [str(n) for n in names]


def _region_entries(regions, nx=None, ny=None, where='regions'):
    """What set_regions / options.region_list is given, checked and completed: a list of 1 to 8 dicts {field, above, below, box,
    name} with above / below as floats (-inf / +inf when absent), box a list of four ints or None (the whole interior) and the
    names distinct (r0, r1, ... when absent).  ValueError, naming the entry, for an unknown key or field, bounds that are no
    numbers, a NaN among them or above >= below, a box that is not four integers ix0 <= ix1, iy0 <= iy1 inside the interior
    (checked against nx, ny where given), a name that is no non-empty string or is used twice.  Host only: no library call."""
    if isinstance(regions, (str, bytes, dict)) or not hasattr(regions, '__len__') or not 1 <= len(regions) <= _lib.REGION_MAX:
        raise ValueError(f"{where}: a list of 1 to {_lib.REGION_MAX} regions {{field, above, below, box, name}} is required, got {regions!r}")
    out = []
    for k, e in enumerate(regions):
        def bad(msg):
            return ValueError(f"{where}: entry {k}: {msg}, got {e!r}")
        if not isinstance(e, dict) or set(e) - {'field', 'above', 'below', 'box', 'name'}:
            raise bad("a dict with the keys field, above, below, box, name is required")
        if e.get('field') not in _lib.REGION_FIELDS:
            raise bad(f"field must be one of {list(_lib.REGION_FIELDS)}")
        bounds = []
        for key, default in (('above', -np.inf), ('below', np.inf)):
            v = e.get(key)
            v = default if v is None else v
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or np.isnan(v):
                raise bad(f"{key} must be a number (inf allowed, NaN not)")
            bounds.append(float(v))
        if not bounds[0] < bounds[1]:
            raise bad("above < below is required (above is inclusive, below exclusive)")
        box = e.get('box')
        if box is not None:
            if isinstance(box, (str, bytes, dict)) or not hasattr(box, '__len__') or len(box) != 4 or \
                    any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) for v in box):
                raise bad("box must be four integers [ix0, ix1, iy0, iy1]")
            box = [int(v) for v in box]
            if not (1 <= box[0] <= box[1] and 1 <= box[2] <= box[3]) or (nx is not None and box[1] > nx) or (ny is not None and box[3] > ny):
                raise bad("box must be ix0 <= ix1 and iy0 <= iy1 inside the interior (inclusive, 1-based)")
        name = e.get('name')
        name = f'r{k}' if name is None else name
        if not isinstance(name, str) or not name:
            raise bad("name must be a non-empty string")
        if name in [o['name'] for o in out]:
            raise bad(f"the name {name!r} is used twice")
        out.append({'field': e['field'], 'above': bounds[0], 'below': bounds[1], 'box': box, 'name': name})
    return out


def _line_centre(along, nx, ny):
    """The reference's centre line: column ny // 2 of the ghosted frame (ny = Ny + 2) along x, row nx // 2 along y."""
    return (ny + 2) // 2 if along == 'x' else (nx + 2) // 2


def _line_span(entry, nx, ny):
    """(first, last) column (along x) or row (along y) of a checked entry, the centre line for at = None."""
    at = entry['at']
    if at is None:
        at = _line_centre(entry['along'], nx, ny)
    return (at, at) if isinstance(at, int) else (at[0], at[1])


def _line_entries(lines, nx=None, ny=None, where='lines'):
    """What set_lines / options.line_list is given, checked and completed: a list of 1 to 8 dicts {along, at, name} with along 'x'
    or 'y', at None (the centre line), an int or a list of two ints, and the names distinct (l0, l1, ... when absent).
    ValueError, naming the entry, for an unknown key or axis, an `at` that is no integer or pair of integers first <= last
    inside the interior (checked against nx, ny where given), a name that is no non-empty string, is used twice or is one of the
    series' own keys.  Host only: no library call."""
    if isinstance(lines, (str, bytes, dict)) or not hasattr(lines, '__len__') or not 1 <= len(lines) <= _lib.LINE_MAX:
        raise ValueError(f"{where}: a list of 1 to {_lib.LINE_MAX} lines {{along, at, name}} is required, got {lines!r}")
    out = []
    for k, e in enumerate(lines):
        def bad(msg):
            return ValueError(f"{where}: entry {k}: {msg}, got {e!r}")

        def is_int(v):
            return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
        if not isinstance(e, dict) or set(e) - {'along', 'at', 'name'}:
            raise bad("a dict with the keys along, at, name is required")
        if e.get('along') not in _lib.LINE_AXES:
            raise bad(f"along must be one of {list(_lib.LINE_AXES)}")
        n = None if nx is None or ny is None else (ny if e['along'] == 'x' else nx)       # the axis `at` counts along
        at = e.get('at')
        if at is not None:
            if is_int(at):
                at = int(at)
                lo = hi = at
            elif not isinstance(at, (str, bytes, dict)) and hasattr(at, '__len__') and len(at) == 2 and all(is_int(v) for v in at):
                at = [int(v) for v in at]
                lo, hi = at
            else:
                raise bad("at must be an integer or a pair of integers (first, last)")
            if not 1 <= lo <= hi or (n is not None and hi > n):
                raise bad("at must be first <= last inside the interior (inclusive, 1-based)")
        name = e.get('name')
        name = f'l{k}' if name is None else name
        if not isinstance(name, str) or not name or name in ('step', 'time', 'names'):
            raise bad("name must be a non-empty string other than step, time, names")
        if name in [o['name'] for o in out]:
            raise bad(f"the name {name!r} is used twice")
        out.append({'along': e['along'], 'at': at, 'name': name})
    return out


def _statistics_fields(fields):
    """The requested fields as a tuple in the library's order; ValueError for anything but a non-empty list of distinct names
    out of p, rho, jx, jy.  Host only: no library call."""
    if isinstance(fields, (str, bytes, dict)) or not hasattr(fields, '__len__') or len(fields) < 1 or \
            not all(isinstance(f, str) and f in _lib.STATS_FIELDS for f in fields) or len(set(fields)) != len(fields):
        raise ValueError(f"statistics: statistics_fields must be a non-empty list of distinct names out of {list(_lib.STATS_FIELDS)}, got {fields!r}")
    return tuple(f for f in _lib.STATS_FIELDS if f in fields)


FRAME_SPEC_KEYS = ('fields', 'window', 'stride', 'reduce', 'dtype', 'capacity')
FRAME_DEFAULT_FIELDS = ('rho', 'jx', 'jy', 'p')


def _frame_spec(given=None, nx=None, ny=None, where='frames'):
    """What set_frames / frame_now / options.frame_spec is given, checked and completed: {fields, window, stride, reduce, dtype,
    capacity} with `fields` a tuple of distinct names of the nine in the library's order (the record's), `window` a list [ix0, ix1,
    iy0, iy1] of inclusive 1-based interior indices or None (the whole interior), `stride` [sx, sy] each in 1..64, `reduce` 'sample'
    or 'mean' -- a mean over blocks of one cell is the cell: 'sample' --, `dtype` 'f4' or 'f8', `capacity` an int >= 1 or None (the
    default).  ValueError for an unknown key, a bad field name, a window outside the interior (checked against nx, ny where given)
    or reversed, a stride outside 1..64, an unknown reduce or dtype, a bad capacity.  Host only: no library call."""
    given = {} if given is None else given

    def bad(msg):
        return ValueError(f"{where}: {msg}, got {given!r}")

    def is_int(v):
        return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))

    def is_list(v, n):
        return not isinstance(v, (str, bytes, dict)) and hasattr(v, '__len__') and len(v) == n
    if not isinstance(given, dict) or set(given) - set(FRAME_SPEC_KEYS):
        raise bad(f"a mapping with the keys {list(FRAME_SPEC_KEYS)} is required")
    fields = given.get('fields')
    fields = FRAME_DEFAULT_FIELDS if fields is None else fields
    if isinstance(fields, (str, bytes, dict)) or not hasattr(fields, '__len__') or len(fields) < 1 or \
            not all(isinstance(f, str) and f in _lib.FRAME_FIELDS for f in fields) or len(set(fields)) != len(fields):
        raise bad(f"fields must be a non-empty list of distinct names out of {list(_lib.FRAME_FIELDS)}")
    window = given.get('window')
    if window is not None:
        if not is_list(window, 4) or not all(is_int(v) for v in window):
            raise bad("window must be four integers [ix0, ix1, iy0, iy1]")
        window = [int(v) for v in window]
        if not (1 <= window[0] <= window[1] and 1 <= window[2] <= window[3]) or (nx is not None and window[1] > nx) or \
                (ny is not None and window[3] > ny):
            raise bad("window must be ix0 <= ix1 and iy0 <= iy1 inside the interior (inclusive, 1-based)")
    stride = given.get('stride')
    stride = (1, 1) if stride is None else stride
    if not is_list(stride, 2) or not all(is_int(v) and 1 <= v <= _lib.FRAME_MAX_STRIDE for v in stride):
        raise bad(f"stride must be two integers [sx, sy] within 1..{_lib.FRAME_MAX_STRIDE}")
    stride = [int(v) for v in stride]
    reduce = given.get('reduce')
    reduce = 'sample' if reduce is None else reduce
    if reduce not in _lib.FRAME_REDUCE:
        raise bad(f"reduce must be one of {list(_lib.FRAME_REDUCE)}")
    if stride == [1, 1]:
        reduce = 'sample'
    dtype = given.get('dtype')
    dtype = 'f4' if dtype is None else dtype
    if dtype not in _lib.FRAME_DTYPES:
        raise bad(f"dtype must be one of {list(_lib.FRAME_DTYPES)}")
    capacity = given.get('capacity')
    if capacity is not None and (not is_int(capacity) or capacity < 1):
        raise bad("capacity must be an integer >= 1 (None: the default)")
    return {'fields': tuple(f for f in _lib.FRAME_FIELDS if f in fields), 'window': window, 'stride': stride, 'reduce': reduce,
            'dtype': dtype, 'capacity': None if capacity is None else int(capacity)}


def _frame_window(spec, nx, ny):
    """(ix0, ix1, iy0, iy1) of a checked spec on an nx x ny interior: its window, or the whole interior."""
    return tuple(spec['window']) if spec['window'] is not None else (1, nx, 1, ny)


def _frame_shape(spec, nx, ny):
    """(mx, my): the blocks of a checked spec's window along x and y, the last of an axis possibly ragged."""
    ix0, ix1, iy0, iy1 = _frame_window(spec, nx, ny)
    sx, sy = spec['stride']
    return -(-(ix1 - ix0 + 1) // sx), -(-(iy1 - iy0 + 1) // sy)


def _frame_axes(spec, nx, ny, dx, dy):
    """(x (mx,), y (my,)): the cell-centre coordinates of a checked spec's output points -- the first cell's for 'sample', the
    mean of the block's cell centres (clipped to the window) for 'mean'."""
    ix0, ix1, iy0, iy1 = _frame_window(spec, nx, ny)
    out = []
    for first, last, s, d in ((ix0, ix1, spec['stride'][0], dx), (iy0, iy1, spec['stride'][1], dy)):
        lo = np.arange(first, last + 1, s)
        hi = np.minimum(lo + s - 1, last) if spec['reduce'] == 'mean' else lo
        out.append((0.5 * (lo + hi) - 0.5) * d)
    return out[0], out[1]
