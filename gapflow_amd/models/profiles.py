"""`GaPFlow.models.profiles` as device operators: get_velocity_profiles / get_stress_profiles (profiles.py:33, 141).

Same signatures, defaults, return order and result shapes as the reference's NumPy broadcasting; the arithmetic runs in
`gpf_gap_profiles_op` (csrc/closures.hpp `profile_coefficients`: the slip parabola of viscous.py's closures evaluated at
every z).  Slip modes as (lower, upper) slip length: both (Ls, Ls), top (0, Ls), bottom (Ls, 0), none (0, 0).

Two forms reach the kernel without copies of q: z shared by every cell -- (nz,) with point inputs, or (nz, 1, ..., 1)
with fields -- and z per cell, (nz,) + the cell shape.  Any other shape the reference accepts (NumPy broadcasting, e.g. a
1-D z against fields whose last axis has nz entries) is broadcast to the full result and evaluated as one level per
element; shapes the reference rejects raise ValueError.  An unknown mode keyword raises ValueError (the reference ends in
UnboundLocalError)."""
import ctypes as C

import numpy as np

from .. import _lib

_Q, _HH, _DQX, _DQY, _ETA, _ZETA, _LS, _Z = range(8)


def _mode_id(mode, keyword):
    if not isinstance(mode, str) or mode not in _lib.PROFILE_MODES:
        raise ValueError(f"{keyword}={mode!r}: expected one of 'both', 'top', 'bottom', 'none'")
    return _lib.PROFILE_MODES[mode]


def _evaluate(z, comps, points, U, V, mode, mask, h_from_z):
    """comps: {bit: array with a leading component axis of >= 3} (None: absent); points: {bit: per-point value}.
    Returns the planes of `mask`, each of the reference's result shape."""
    lib = _lib.require_device()
    z = np.asarray(z, dtype=float)
    if z.ndim == 0:
        raise ValueError("z must be an array of levels")
    comps = {b: np.asarray(a, dtype=float)[:3] for b, a in comps.items() if a is not None}
    for b, a in comps.items():
        if a.shape[0] != 3:
            raise ValueError(f"expected 3 components, got shape {a.shape}")
    points = {b: np.asarray(a, dtype=float) for b, a in points.items()}
    S = np.broadcast_shapes(*[a.shape[1:] for a in comps.values()], *[a.shape for a in points.values()])
    O = np.broadcast_shapes(z.shape, S)         # the reference's result shape (ValueError where NumPy refuses)
    nz = z.shape[0]
    fits = len(S) <= z.ndim - 1 and z.ndim == len(O)
    if fits and z.size == nz:                   # one z column for every cell
        cells, zin, per_cell = O[1:], z.reshape(nz), 0
    elif fits and z.shape == O:                 # a z column per cell
        cells, zin, per_cell = O[1:], z, 1 << _Z
    else:                                       # general broadcast: every element of the result is a cell with one level
        if h_from_z:                            # (the velocity profile's gap height is z[-1] of the z it was given)
            comps[_HH] = np.stack(np.broadcast_arrays(z[-1], 0.0, 0.0))
        cells, nz, zin, per_cell = O, 1, np.broadcast_to(z, O), 1 << _Z
        h_from_z = False
    n = int(np.prod(cells, dtype=np.int64)) if cells else 1
    args = {}
    for b, a in list(comps.items()) + list(points.items()):
        lead = a.shape[:1] if b in comps else ()
        cs = a.shape[len(lead):]
        if int(np.prod(cs, dtype=np.int64)) == 1:
            args[b] = _lib.f64c(a.reshape(lead + (1,))[..., 0] if lead else a.reshape(1))
        else:
            if (1,) * (len(cells) - len(cs)) + cs != tuple(cells):
                a = np.broadcast_to(a, lead + tuple(cells))     # partial broadcast (e.g. (nx, 1) against (nx, ny))
            args[b] = _lib.f64c(a).reshape(lead + (n,))
            per_cell |= 1 << b
    zin = _lib.f64c(zin)
    nplanes = sum(1 if m != _lib.PROFILE_TAU else 6 for m in (_lib.PROFILE_Z, _lib.PROFILE_U, _lib.PROFILE_V, _lib.PROFILE_TAU)
                  if mask & m)
    out = np.empty((nplanes, nz, n))
    ptr = lambda b: args[b].ctypes.data_as(C.c_void_p) if b in args else None
    _lib.check(lib.gpf_gap_profiles_op(n, nz, zin.ctypes.data_as(C.c_void_p), ptr(_Q), None if h_from_z else ptr(_HH),
                                       ptr(_DQX), ptr(_DQY), ptr(_ETA), ptr(_ZETA), ptr(_LS), per_cell, float(U), float(V),
                                       mode, mask, out.ctypes.data_as(C.c_void_p)))
    return tuple(out[k].reshape(O) for k in range(nplanes))


def get_velocity_profiles(z, q, Ls=0.0, U=1.0, V=0.0, slip="both"):
    """Velocity profiles u(z), v(z) for the gap-averaged solution q = (rho, jx, jy) (profiles.py:33-138).  As in the
    reference the gap height is z[-1]."""
    mode = _mode_id(slip, 'slip')
    return _evaluate(z, {_Q: q}, {_LS: Ls, _ETA: 0.0, _ZETA: 0.0}, U, V, mode, _lib.PROFILE_U | _lib.PROFILE_V, True)


def get_stress_profiles(z, h, q, dqx, dqy, U=1.0, V=0.0, eta=1.0, zeta=1.0, Ls=0, mode="both"):
    """Viscous stress profiles tau_xx, tau_yy, tau_zz, tau_yz, tau_xz, tau_xy at z (profiles.py:141-1323); h = (h, dh/dx,
    dh/dy), dqx / dqy the x / y gradients of q."""
    m = _mode_id(mode, 'mode')
    return _evaluate(z, {_Q: q, _HH: h, _DQX: dqx, _DQY: dqy}, {_ETA: eta, _ZETA: zeta, _LS: Ls}, U, V, m,
                     _lib.PROFILE_TAU, False)
