"""Elastic deformation of the gap under the film pressure (GaPFlow/topography.py:257-271, 327-437).

The reference hands the half-space response to ContactMechanics (FFT-based Green's functions); here the Green's function
is assembled once on the host, its Fourier transform lives on the device, and every time step the convolution
p -> u runs there (hipFFT real-to-complex transforms + small kernels, `gpf_elastic_update`), followed by the
under-relaxation, h = h_undeformed + u and the np.gradient stencil for dh/dx, dh/dy.

PARITY UNPINNED against ContactMechanics (not installed here, no fixture or test in the reference): the three response
functions follow the published forms -- periodic: u(q) = 2 p(q) / (E* |q|) with the q = 0 mode removed (Johnson,
Greenwood & Higginson 1985); free: Love's uniformly loaded rectangle on a doubled grid (Johnson 1985, eq. 3.25; Hockney &
Eastwood); semi-periodic: the free response summed over `n_images` periodic images on either side -- and the conventions of
the reference's wrapper (grid incl. ghost cells on (Lx, Ly), forces p dx dy, positive pressure -> positive displacement,
reference point [0, 0] subtracted unless fully periodic).  tests/test_oracle_elastic.py pins the same forms to analytic
solutions."""
import ctypes as C
import warnings

import numpy as np

from . import _lib


def _love(x, y, a, b, young):
    def term(p, q1, q2):
        return p * np.log((q1 + np.sqrt(q1 * q1 + p * p)) / (q2 + np.sqrt(q2 * q2 + p * p)))
    return (term(x + a, y + b, y - b) + term(y + b, x + a, x - a)
            + term(x - a, y - b, y + b) + term(y - b, x - a, x + a)) / (np.pi * young)


class ElasticDeformation:
    """Host half: which half-space applies, its Green's function in Fourier space, and the hand-over to the device."""

    def __init__(self, E, v, alpha_underrelax, grid, n_images):
        self.area_per_cell = grid['dx'] * grid['dy']
        nx, ny = grid['Nx'] + 2, grid['Ny'] + 2
        self.alpha_underrelax = alpha_underrelax
        perX, perY = bool(grid['bc_xE_P'][0]), bool(grid['bc_yS_P'][0])
        young_effective = E / (1 - v**2)
        Lx, Ly = grid['Lx'], grid['Ly']
        if (perX != perY) and ((perY and grid['Ny'] == 1) or (perX and grid['Nx'] == 1)):
            warnings.warn("You specified a semi-periodic 1D problem.\n"
                          "For the calculation of elastic deformation, we assume a line contact with "
                          "non-periodic boundary conditions in both directions.\n"
                          "For the calculation of the effective force F=p*A per cell, "
                          "we assume a unit length of {} = 1.".format("Ly" if perY else "Lx"))
            if perY:
                Ly = 1.0
            else:
                Lx = 1.0
            n_images = 0
        sx, sy = Lx / nx, Ly / ny
        self.area_per_pt = sx * sy
        if perX and perY:
            self.periodicity = 'full'
            self.shape_fft = (nx, ny)
            q = np.hypot(np.fft.fftfreq(nx, d=sx)[:, None], np.fft.rfftfreq(ny, d=sy)[None, :])
            with np.errstate(divide='ignore'):
                self.greens = np.where(q > 0, 1.0 / (np.pi * young_effective * q), 0.0).astype(complex)
            self._G_real = None
        else:
            self.periodicity = 'half' if perX != perY else 'none'
            if self.periodicity == 'none':
                n_images = 0
            px, py = (nx if perX else 2 * nx), (ny if perY else 2 * ny)
            self.shape_fft = (px, py)
            ix, iy = np.arange(px), np.arange(py)
            xs = (np.where(ix <= nx // 2, ix, ix - nx) if perX else np.where(ix <= nx, ix, ix - 2 * nx)) * sx
            ys = (np.where(iy <= ny // 2, iy, iy - ny) if perY else np.where(iy <= ny, iy, iy - 2 * ny)) * sy
            G = np.zeros((px, py))
            for k in range(-n_images, n_images + 1):
                G += _love(xs[:, None] + (k * Lx if perX else 0.0), ys[None, :] + (k * Ly if perY else 0.0),
                           sx / 2, sy / 2, young_effective)
            self._G_real = G
            self.greens = np.fft.rfft2(G)

    def attach(self, problem):
        """Upload the Green's function; from now on gpf_elastic_update(problem) deforms the gap on the device."""
        g = np.ascontiguousarray(np.stack([self.greens.real, self.greens.imag], axis=-1), dtype=np.float64)
        px, py = self.shape_fft
        _lib.check(problem._lib.gpf_elastic_setup(problem._h, px, py, g.ctypes.data_as(C.c_void_p), g.size,
                                                  float(self.alpha_underrelax), float(self.area_per_cell / self.area_per_pt),
                                                  0 if self.periodicity == 'full' else 1))

    def attach_slab(self, problem, plan, rank, h0_rows):
        """Upload this rank's share for the x-slab form (gpf_elastic_slab_setup): its ky slab of the Green's spectrum (the
        whole spectrum is never resident on the device) and the undeformed gap of the rows it gets back."""
        px, py = self.shape_fft
        k0, nk = plan.ky[rank]
        g = np.ascontiguousarray(np.stack([self.greens.real[:, k0:k0 + nk], self.greens.imag[:, k0:k0 + nk]], axis=-1),
                                 dtype=np.float64)
        ints = plan.c_plan(rank)
        h0 = np.ascontiguousarray(h0_rows, dtype=np.float64)
        _lib.check(problem.lib.gpf_elastic_slab_setup(problem._h, px, py, plan.world, ints.ctypes.data_as(C.c_void_p), ints.size,
                                                      g.ctypes.data_as(C.c_void_p), g.size, h0.ctypes.data_as(C.c_void_p), h0.size,
                                                      float(self.alpha_underrelax), float(self.area_per_cell / self.area_per_pt),
                                                      0 if self.periodicity == 'full' else 1))

    # -- analysis helpers of the reference (topography.py:439-465) -----------------------------
    def get_G_real(self):
        if self._G_real is None:
            raise NotImplementedError("the periodic half-space is defined in Fourier space only")
        return np.fft.fftshift(self._G_real)

    def get_G_real_slices(self):
        G = self.get_G_real()
        return G[:, G.shape[1] // 2], G[G.shape[0] // 2, :]


def ky_partition(nky, world):
    """(k0, nk) of every rank: [0, nky) cut into `world` consecutive slabs, the first nky % world one column wider; a rank
    may get none (csrc/elastic_kernels.hip: KySplit)."""
    base, rem = divmod(nky, world)
    out, k0 = [], 0
    for r in range(world):
        n = base + (1 if r < rem else 0)
        out.append((k0, n))
        k0 += n
    return out


class SlabElasticPlan:
    """Who transforms, holds and receives what in the x-slab form of the half-space convolution (plain Python; the
    device side is csrc/api_slab_elastic.inc).  Rows are global indices 0..Nx+1 of the (Nx+2)-row field, slabs are the
    `parts` of slab.partition (contiguous in x, in rank order); the transform grid is px x py with nky = py/2 + 1 columns.

      fwd[r]   = (row0, nrows)  transform rows rank r owns: its interior rows, + row 0 on the first rank, + row Nx+1 on the
                                last.  The zero rows of a doubled x range are never transformed or sent.
      ky[r]    = (k0, nk)       its ky column slab (ky_partition)
      main[r]  = (g0, n)        rows it gets back: lo-2 .. hi+2 clipped to [0, Nx+1] -- its rows and the one beyond each,
                                so that np.gradient is exact on all of them
      seam[r]  = (side, g0)     on a periodic seam edge (world > 1): three more rows across the seam, Nx-1..Nx+1 for the
                                first rank (side 0), 0..2 for the last (side 1); (-1, 0) elsewhere
    Split sizes of the two all-to-alls are in complex numbers (two doubles each)."""

    def __init__(self, Nx, px, py, parts, seam):
        self.Nx, self.px, self.py, self.nky = Nx, px, py, py // 2 + 1
        self.parts, self.world = list(parts), len(parts)
        last = self.world - 1
        self.fwd, self.main, self.seam = [], [], []
        for r, (lo, hi) in enumerate(self.parts):
            r0, r1 = (0 if r == 0 else lo), (Nx + 1 if r == last else hi)
            self.fwd.append((r0, r1 - r0 + 1))
            m0, m1 = max(0, lo - 2), min(Nx + 1, hi + 2)
            self.main.append((m0, m1 - m0 + 1))
            if seam and self.world > 1 and r == 0:
                self.seam.append((0, Nx - 1))
            elif seam and self.world > 1 and r == last:
                self.seam.append((1, 0))
            else:
                self.seam.append((-1, 0))
        self.ky = ky_partition(self.nky, self.world)

    @classmethod
    def for_grid(cls, grid, world, shape_fft):
        from .slab import partition
        periodic = all(grid['bc_xE_P']) and all(grid['bc_xW_P'])
        return cls(grid['Nx'], shape_fft[0], shape_fft[1], partition(grid['Nx'], world), periodic)

    def return_rows(self, r):
        g0, n = self.main[r]
        rows = list(range(g0, g0 + n))
        side, s0 = self.seam[r]
        if side >= 0:
            rows += [s0, s0 + 1, s0 + 2]
        return rows

    def send1(self, r):
        return [self.fwd[r][1] * self.ky[s][1] for s in range(self.world)]

    def recv1(self, r):
        return [self.fwd[s][1] * self.ky[r][1] for s in range(self.world)]

    def send2(self, r):
        return [len(self.return_rows(s)) * self.ky[r][1] for s in range(self.world)]

    def recv2(self, r):
        return [len(self.return_rows(r)) * self.ky[s][1] for s in range(self.world)]

    def c_plan(self, r):
        """int32 plan of rank r in the layout of gpf_elastic_slab_setup."""
        lo, hi = self.parts[r]
        rows_all = [g for s in range(self.world) for g in self.return_rows(s)]
        head = [self.fwd[r][0], self.fwd[r][1], self.ky[r][0], self.ky[r][1], len(self.return_rows(r)), self.main[r][1],
                self.main[r][0], self.seam[r][0], self.seam[r][1], len(rows_all), lo - 1, self.Nx, r]
        return np.asarray(head + rows_all, dtype=np.int32)
