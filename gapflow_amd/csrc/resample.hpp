// Resampling a state onto another grid of the same domain (entry point: api_resample.inc, kernel: resample_kernels.hip).
// Plain C++ when compiled without hipcc, like closures.hpp: tests/hostcheck/resample_host.cpp builds it with g++ under the
// sanitizers and holds it against NumPy.
//
// Bilinear interpolation over the source's GHOSTED cell centres, at the destination's interior cell centres.  Along one axis,
// destination cell i = 1..n_dst sits at (i - 1/2) d_dst, source cell k = 0..n_src+1 at (k - 1/2) d_src, so in units of source cells
//     s = (i - 1/2) (d_dst / d_src) + 1/2,     i0 = floor(s) clamped to 0..n_src,     w = s - i0,
//     value = (1 - w) f[i0] + w f[i0 + 1].
// Both grids cover the same length, so 1/2 < s < n_src + 1/2: the two cells always exist (the clamp guards the last bit only)
// and no edge is special -- the ghost cells hold the periodic image or the Dirichlet / Neumann value.  An axis of extent 1 on
// both sides takes the single interior line with weight 0.
// Interpolated are rho and the flow rates per width jx h, jy h with the SOURCE's gap (what a steady film keeps smooth; in 1-D
// jx h is constant); the destination's momenta are these divided by ITS gap.
// Every contraction that decides a rounding is written out as fma: s is ONE rounding of the exact (i - 1/2) ratio + 1/2
// (gapflow_amd/resample.py: axis_weights reproduces it exactly), a blend is (1 - w) f0 rounded, then one fma.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define GPF_RS_HD __host__ __device__ __forceinline__
#else
#define GPF_RS_HD inline
#endif

namespace gpf {

struct ResampleAxis {
    int i0;         // lower source cell of the pair, ghosted index 0..n_src
    double w;       // weight of cell i0 + 1, in [0, 1)
};

// Destination cell i (1..n_dst) along one axis; ratio = d_dst / d_src; unit: the axis has extent 1 on both sides
GPF_RS_HD ResampleAxis resample_axis(int i, double ratio, int n_src, bool unit) {
    ResampleAxis a;
    if (unit) { a.i0 = 1; a.w = 0.0; return a; }
    const double s = fma((double)i - 0.5, ratio, 0.5);
    double f = floor(s);
    if (!(f >= 0.0)) f = 0.0;
    if (f > (double)n_src) f = (double)n_src;
    a.i0 = (int)f;
    a.w = s - f;
    return a;
}

GPF_RS_HD double resample_lerp(double f0, double f1, double w) {
    const double a = (1.0 - w) * f0;
    return fma(w, f1, a);
}

// Corners in the order (i0, j0), (i0, j0 + 1), (i0 + 1, j0), (i0 + 1, j0 + 1); wx along the first index, wy along the second
GPF_RS_HD double resample_blend(const double f[4], double wx, double wy) {
    return resample_lerp(resample_lerp(f[0], f[1], wy), resample_lerp(f[2], f[3], wy), wx);
}

struct ResampleOut { double rho, jx, jy; };

// One destination cell from the four source corners of rho, jx, jy and the source's gap h, and the destination's own gap
GPF_RS_HD ResampleOut resample_cell(const double rho[4], const double jx[4], const double jy[4], const double h[4], double wx, double wy,
                                    double h_dst) {
    const double fx[4] = {jx[0] * h[0], jx[1] * h[1], jx[2] * h[2], jx[3] * h[3]};
    const double fy[4] = {jy[0] * h[0], jy[1] * h[1], jy[2] * h[2], jy[3] * h[3]};
    ResampleOut o;
    o.rho = resample_blend(rho, wx, wy);
    o.jx = resample_blend(fx, wx, wy) / h_dst;
    o.jy = resample_blend(fy, wx, wy) / h_dst;
    return o;
}

}  // namespace gpf
