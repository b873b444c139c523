"""Weight planes for Problem.set_weighted_integrals: interior (Nx, Ny) arrays for a problem's `grid` dictionary.

    box(grid, ix0, ix1, iy0, iy1)       1.0 inside the inclusive index ranges, 0.0 outside: one pad, one asperity, a window
    mode(grid, kx, ky, phase)           one Fourier mode of the domain, evaluated at the cell centres
    load(path)                          a plane (or a stack of planes) from an .npy file

Indices are interior and 1-based, as everywhere in this package: row ix of the ghosted field is row ix - 1 of a plane.
Host only: nothing here touches the device."""
import os

import numpy as np


def _extent(grid):
    return int(grid['Nx']), int(grid['Ny'])


def _index(v, what):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"weights: {what} must be an integer, got {v!r}")
    return int(v)


def box(grid, ix0, ix1, iy0, iy1):
    """1.0 on the interior cells ix0 <= ix <= ix1, iy0 <= iy <= iy1 (inclusive, 1-based), exactly 0.0 elsewhere.
    ValueError for a range that is empty or leaves the interior 1..Nx x 1..Ny."""
    nx, ny = _extent(grid)
    ix0, ix1, iy0, iy1 = (_index(v, n) for v, n in ((ix0, 'ix0'), (ix1, 'ix1'), (iy0, 'iy0'), (iy1, 'iy1')))
    if not 1 <= ix0 <= ix1 <= nx:
        raise ValueError(f"weights: box rows {ix0}..{ix1} must satisfy 1 <= ix0 <= ix1 <= {nx}")
    if not 1 <= iy0 <= iy1 <= ny:
        raise ValueError(f"weights: box columns {iy0}..{iy1} must satisfy 1 <= iy0 <= iy1 <= {ny}")
    w = np.zeros((nx, ny))
    w[ix0 - 1:ix1, iy0 - 1:iy1] = 1.0
    return w


def mode(grid, kx, ky, phase='cos'):
    """cos or sin of 2 pi (kx x / Lx + ky y / Ly) at the cell centres x = (ix - 1/2) dx, y = (iy - 1/2) dy, with Lx = Nx dx and
    Ly = Ny dy: the weighted integral of rho with this plane is Lx Ly / 2 times the amplitude of that mode of rho."""
    nx, ny = _extent(grid)
    kx, ky = _index(kx, 'kx'), _index(ky, 'ky')
    if phase not in ('cos', 'sin'):
        raise ValueError(f"weights: phase must be 'cos' or 'sin', got {phase!r}")
    dx, dy = float(grid['dx']), float(grid['dy'])
    x = (np.arange(1, nx + 1) - 0.5) * dx
    y = (np.arange(1, ny + 1) - 0.5) * dy
    arg = 2.0 * np.pi * (kx * x[:, None] / (nx * dx) + ky * y[None, :] / (ny * dy))
    return np.cos(arg) if phase == 'cos' else np.sin(arg)


def load(path):
    """The array an .npy file holds, as float64: (Nx, Ny) for one plane or (K, Nx, Ny) for several (set_weighted_integrals checks
    the shape against its grid)."""
    a = np.load(os.fspath(path), allow_pickle=False)
    if a.ndim not in (2, 3):
        raise ValueError(f"weights: {path} holds an array of shape {a.shape}; (Nx, Ny) or (K, Nx, Ny) required")
    return np.ascontiguousarray(a, dtype=np.float64)


def parse_entries(entries, grid=None, base_dir=None):
    """`options.weights` as a list of plain dictionaries {'box': [ix0, ix1, iy0, iy1]} / {'mode': [kx, ky, phase]} /
    {'file': absolute path}, each with a 'name'.  ValueError naming the entry for anything else; a box is checked against
    `grid` when the input has one.  A relative `file` is relative to `base_dir` (the YAML file's directory; none: the working
    directory).  Host only: files are not opened here."""
    if isinstance(entries, (str, bytes, dict)) or not hasattr(entries, '__len__') or len(entries) < 1:
        raise ValueError(f"options.weights: a non-empty list of {{box: ...}} / {{mode: ...}} / {{file: ...}} entries is required, got {entries!r}")
    out = []
    for k, e in enumerate(entries):
        kinds = [key for key in ('box', 'mode', 'file') if isinstance(e, dict) and key in e]
        if len(kinds) != 1 or set(e) - {'box', 'mode', 'file', 'name'}:
            raise ValueError(f"options.weights: entry {k} must hold exactly one of box, mode, file (and an optional name), got {e!r}")
        kind, v = kinds[0], e[kinds[0]]
        name = e.get('name', f'w{k}')
        if not isinstance(name, str) or not name:
            raise ValueError(f"options.weights: entry {k}: name must be a non-empty string, got {name!r}")
        try:
            if kind == 'box':
                if isinstance(v, (str, bytes, dict)) or not hasattr(v, '__len__') or len(v) != 4:
                    raise ValueError(f"box needs [ix0, ix1, iy0, iy1], got {v!r}")
                v = [_index(x, 'a box index') for x in v]
                if grid is not None and 'Nx' in grid and 'Ny' in grid:
                    box(grid, *v)
            elif kind == 'mode':
                if isinstance(v, (str, bytes, dict)) or not hasattr(v, '__len__') or len(v) not in (2, 3):
                    raise ValueError(f"mode needs [kx, ky] or [kx, ky, cos|sin], got {v!r}")
                v = [_index(v[0], 'kx'), _index(v[1], 'ky'), v[2] if len(v) == 3 else 'cos']
                if v[2] not in ('cos', 'sin'):
                    raise ValueError(f"the phase must be cos or sin, got {v[2]!r}")
            else:
                if not isinstance(v, str) or not v:
                    raise ValueError(f"file needs the path of an .npy file, got {v!r}")
                v = os.path.normpath(os.path.join(base_dir or os.getcwd(), v))
        except ValueError as err:
            raise ValueError(f"options.weights: entry {k}: {err}") from None
        out.append({kind: v, 'name': name})
    return out


def from_entries(grid, entries):
    """(planes (K, Nx, Ny), names) of parse_entries' output: a file that holds several planes contributes them all, named
    name_0, name_1, ..."""
    planes, names = [], []
    for k, e in enumerate(entries):
        if 'box' in e:
            planes.append(box(grid, *e['box'])); names.append(e['name'])
        elif 'mode' in e:
            planes.append(mode(grid, *e['mode'])); names.append(e['name'])
        else:
            a = load(e['file'])
            if a.shape[-2:] != _extent(grid):
                raise ValueError(f"options.weights: entry {k}: {e['file']} holds planes of shape {a.shape[-2:]}, the grid is {_extent(grid)}")
            if a.ndim == 2:
                planes.append(a); names.append(e['name'])
            else:
                planes.extend(a); names.extend(f"{e['name']}_{j}" for j in range(len(a)))
    return np.stack(planes), names
