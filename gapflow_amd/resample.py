"""Host side of resampling a state onto another grid (``Problem.init_from``, gpf_resample): the index and
weight rule as NumPy code, and the refusals that need no device.  The arithmetic on fields runs in the library only."""
from fractions import Fraction

import numpy as np

LENGTH_RTOL = 1e-12         # Lx, Ly of source and destination may differ by this much, relative (gpf_resample's bound)


def axis_weights(n_dst, d_dst, d_src, n_src=None):
    """(i0, w) for the destination cells i = 1..n_dst of one axis: the lower source cell of the pair, a ghosted index
    0..n_src, and the weight of cell i0 + 1, in [0, 1) -- value = (1 - w) f[i0] + w f[i0 + 1].

        s = (i - 1/2) (d_dst / d_src) + 1/2,    i0 = floor(s) clamped to 0..n_src,    w = s - i0

    with s rounded ONCE from the exact product and sum, as the library's fma does (csrc/resample.hpp: resample_axis): indices
    and weights are the library's bit for bit.  n_src defaults to the cell count of the same length, round(n_dst d_dst / d_src).
    An axis of extent 1 on both sides copies the single interior line: i0 = 1, w = 0."""
    n_dst = int(n_dst)
    if n_dst < 1 or not d_dst > 0 or not d_src > 0:
        raise ValueError(f"axis_weights: n_dst >= 1 and positive spacings required, got {n_dst}, {d_dst!r}, {d_src!r}")
    if n_src is None:
        n_src = int(round(n_dst * float(d_dst) / float(d_src)))
    n_src = int(n_src)
    if n_src < 1:
        raise ValueError(f"axis_weights: the source axis has no cell (n_src = {n_src})")
    if n_dst == 1 and n_src == 1:
        return np.ones(1, dtype=np.int64), np.zeros(1)
    ratio = Fraction(float(d_dst) / float(d_src))       # the double the library divides out, exactly
    half = Fraction(1, 2)
    s = np.array([float((Fraction(i) - half) * ratio + half) for i in range(1, n_dst + 1)])
    f = np.clip(np.floor(s), 0.0, float(n_src))
    return f.astype(np.int64), s - f


def geometry_refusal(grid_dst, grid_src):
    """Why a state on `grid_src` cannot be resampled onto `grid_dst` (sanitised grid dictionaries), or None: the domains must
    agree to LENGTH_RTOL and each direction must be periodic on both sides or on neither.  Host only."""
    for k, n, d in (('Lx', 'Nx', 'dx'), ('Ly', 'Ny', 'dy')):
        a, b = (float(g[n]) * float(g[d]) for g in (grid_src, grid_dst))
        if abs(a - b) > LENGTH_RTOL * max(abs(a), abs(b)):
            return f"the domains differ: {k} = {a!r} on the source, {b!r} on the destination"
    for axis, edges in (('x', ('xE', 'xW')), ('y', ('yS', 'yN'))):
        for e in edges:
            ps, pd = all(grid_src[f'bc_{e}_P']), all(grid_dst[f'bc_{e}_P'])
            if ps != pd:
                return (f"the {axis} direction (edge {e}) is periodic on the {'source' if ps else 'destination'} and not on the "
                        f"{'destination' if ps else 'source'}")
    return None


def check_geometry(grid_dst, grid_src):
    """ValueError naming why a state on `grid_src` cannot be resampled onto `grid_dst`; nothing when it can.  Host only."""
    why = geometry_refusal(grid_dst, grid_src)
    if why:
        raise ValueError(f"init_from: {why}")


def check_axes(grid_dst, grid_src):
    """The index and weight tables of both axes, checked: every pair of source cells exists and every weight lies in [0, 1)."""
    out = []
    for n, d in (('Nx', 'dx'), ('Ny', 'dy')):
        i0, w = axis_weights(grid_dst[n], grid_dst[d], grid_src[d], grid_src[n])
        if i0.min() < 0 or i0.max() > grid_src[n] or w.min() < 0.0 or not w.max() < 1.0:
            raise ValueError(f"init_from: the {n[1]} axes do not cover the same length ({grid_src[n]} cells of {grid_src[d]!r} -> "
                             f"{grid_dst[n]} cells of {grid_dst[d]!r})")
        out.append((i0, w))
    return out
