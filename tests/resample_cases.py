"""Shared by tests/test_resample_host.py and tests/test_gpu_resample.py: the NumPy restatement of resampling a state onto another
grid -- gapflow_amd.resample.axis_weights, then the four-term blend, then the division by the destination's
gap -- and the 2-D grid pairs both files run."""
import numpy as np

from gapflow_amd.resample import axis_weights

# (source Nx, Ny) -> (destination Nx, Ny) of the 2-D cases: non-integer ratios with an odd destination Ny; 2.5 x 3; coarsening;
# a destination beyond 1200 ghosted cells; identity
GRID_PAIRS = {'b': ((12, 10), (30, 25)), 'c': ((16, 8), (40, 24)), 'd': ((30, 25), (12, 10)), 'e': ((12, 10), (48, 40)), 'f': ((16, 8), (16, 8))}


def blend(f, ix0, wx, iy0, wy):
    """Bilinear blend of the ghosted field f at the tabulated pairs: along y first, then along x."""
    i0, j0 = ix0[:, None], iy0[None, :]
    wy = wy[None, :]
    wx = wx[:, None]
    a = (1.0 - wy) * f[i0, j0] + wy * f[i0, j0 + 1]
    b = (1.0 - wy) * f[i0 + 1, j0] + wy * f[i0 + 1, j0 + 1]
    return (1.0 - wx) * a + wx * b


def numpy_resample(q_src, h_src, h_dst, d_src, d_dst):
    """The destination's interior (3, Nx_d, Ny_d) from the source's ghosted state (3, Nx_s + 2, Ny_s + 2), the source's ghosted gap
    and the destination's ghosted gap; d_src, d_dst = (dx, dy)."""
    nxs, nys = q_src.shape[1] - 2, q_src.shape[2] - 2
    nxd, nyd = h_dst.shape[0] - 2, h_dst.shape[1] - 2
    ix0, wx = axis_weights(nxd, d_dst[0], d_src[0], nxs)
    iy0, wy = axis_weights(nyd, d_dst[1], d_src[1], nys)
    hd = h_dst[1:-1, 1:-1]
    return np.stack([blend(q_src[0], ix0, wx, iy0, wy),
                     blend(q_src[1] * h_src, ix0, wx, iy0, wy) / hd,
                     blend(q_src[2] * h_src, ix0, wx, iy0, wy) / hd])


def fill_ghosts(interior, rules, values):
    """The ghosted field (3, Nx + 2, Ny + 2) of an interior (3, Nx, Ny) by the edge rules of Problem._edge_rules (0 periodic,
    1 Dirichlet, 2 Neumann; edges ix = 0, ix = Nx + 1, iy = 0, iy = Ny + 1): x edges over the interior columns, then y edges over
    all rows, so that the corners are rule_y(rule_x(.))."""
    nx, ny = interior.shape[1:]
    q = np.zeros((3, nx + 2, ny + 2))
    q[:, 1:-1, 1:-1] = interior
    for c in range(3):
        for e, (ghost, adj, far) in enumerate(((0, 1, nx), (nx + 1, nx, 1))):
            r = rules[e][c]
            v = q[c, far if r == 0 else adj, :]
            q[c, ghost, :] = 2.0 * values[e] - v if r == 1 else v
        for e, (ghost, adj, far) in ((2, (0, 1, ny)), (3, (ny + 1, ny, 1))):
            r = rules[e][c]
            v = q[c, :, far if r == 0 else adj]
            q[c, :, ghost] = 2.0 * values[e] - v if r == 1 else v
    return q
