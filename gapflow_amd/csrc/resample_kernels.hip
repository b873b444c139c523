// k_resample: the interior of a destination state from a source state on another grid of the same domain (arithmetic:
// resample.hpp, entry point: api_resample.inc).  Per destination cell 3 doubles are written and 1 is read (its gap); the 16
// source values behind a cell come from the -- normally smaller -- source grid, which sits in cache, and neighbouring
// destination cells share them.  Meant to be store-bound; measured at 1024^2 -> 4096^2 it takes three times a kernel that only
// stores the same bytes (profiles/resample/README.md), so the loads and the arithmetic still show.
//
// The geometry of k_film_partial / k_extrema_partial: one 256-thread workgroup per destination interior row, thread t owns the
// column pairs (1 + 2k, 2 + 2k) for k = t, t + 256, ...  The row's source index and weight are block-uniform; a lane works out
// the column indices and weights of its pair once and uses them for all four source planes.  A whole pair is written with one
// 16-byte store per plane where the destination's buffers allow it (film_wide_ok's conditions; `wide`), with 8-byte stores
// otherwise; the single cell an odd Ny leaves in the last pair is always an 8-byte store, so that no ghost cell is written here
// (the ghost cells are k_bc_x / k_bc_y's, launched behind this kernel).  Source reads go through the source's Layout as plain
// addresses, whatever pieces back its fields.
#pragma once

#include "device_types.hpp"
#include "resample.hpp"

namespace gpf {

typedef double rs_d2 __attribute__((ext_vector_type(2)));

struct ResampleArgs {
    const double* sq;       // the source's committed state, 3 planes of Ls
    const double* sh;       // the source's gap height (plane 0 of its gap planes)
    double* dq;             // the destination's state buffer, 3 planes of Ld
    const double* dh;       // the destination's gap height
    Layout Ls, Ld;
    double rx, ry;          // dx_dst / dx_src, dy_dst / dy_src
    int unit_x, unit_y;     // the axis has extent 1 on both sides
    int wide;
};

__device__ __forceinline__ ResampleOut resample_at(const ResampleArgs& a, const ResampleAxis& ax, const ResampleAxis& ay, double h_dst) {
    const long long o0 = a.Ls.at(ax.i0, ay.i0), o1 = o0 + a.Ls.pitch;
    const double* jxp = a.sq + a.Ls.plane;
    const double* jyp = jxp + a.Ls.plane;
    const double rho[4] = {a.sq[o0], a.sq[o0 + 1], a.sq[o1], a.sq[o1 + 1]};
    const double jx[4] = {jxp[o0], jxp[o0 + 1], jxp[o1], jxp[o1 + 1]};
    const double jy[4] = {jyp[o0], jyp[o0 + 1], jyp[o1], jyp[o1 + 1]};
    const double h[4] = {a.sh[o0], a.sh[o0 + 1], a.sh[o1], a.sh[o1 + 1]};
    return resample_cell(rho, jx, jy, h, ax.w, ay.w, h_dst);
}

__global__ __launch_bounds__(256) void k_resample(const ResampleArgs a) {
    const int ix = 1 + blockIdx.x;
    if (ix > a.Ld.Nx) return;
    const ResampleAxis ax = resample_axis(ix, a.rx, a.Ls.Nx, a.unit_x != 0);
    const int npair = (a.Ld.Ny + 1) / 2;
    double* const out0 = a.dq;
    double* const out1 = a.dq + a.Ld.plane;
    double* const out2 = out1 + a.Ld.plane;
    for (int k = threadIdx.x; k < npair; k += 256) {
        const int iy = 1 + 2 * k;
        const bool two = iy + 1 <= a.Ld.Ny;
        const long long o = a.Ld.at(ix, iy);
        const ResampleAxis ay0 = resample_axis(iy, a.ry, a.Ls.Ny, a.unit_y != 0);
        const ResampleAxis ay1 = resample_axis(two ? iy + 1 : iy, a.ry, a.Ls.Ny, a.unit_y != 0);
        double h0, h1;
        if (a.wide) {       // (the ghost column an odd Ny reaches is loaded and not used)
            const rs_d2 hd = *reinterpret_cast<const rs_d2*>(a.dh + o);
            h0 = hd.x; h1 = two ? hd.y : hd.x;
        } else {
            h0 = a.dh[o]; h1 = two ? a.dh[o + 1] : h0;
        }
        const ResampleOut c0 = resample_at(a, ax, ay0, h0);
        const ResampleOut c1 = resample_at(a, ax, ay1, h1);
        if (a.wide && two) {
            *reinterpret_cast<rs_d2*>(out0 + o) = rs_d2{c0.rho, c1.rho};
            *reinterpret_cast<rs_d2*>(out1 + o) = rs_d2{c0.jx, c1.jx};
            *reinterpret_cast<rs_d2*>(out2 + o) = rs_d2{c0.jy, c1.jy};
        } else {
            out0[o] = c0.rho; out1[o] = c0.jx; out2[o] = c0.jy;
            if (two) { out0[o + 1] = c1.rho; out1[o + 1] = c1.jx; out2[o + 1] = c1.jy; }
        }
    }
}

// The store stream of k_resample alone (tools/resample_time.py): the same rows, pairs and stores of a constant, no source reads
__global__ __launch_bounds__(256) void k_resample_store_only(double* dq, const Layout Ld, int wide, double value) {
    const int ix = 1 + blockIdx.x;
    if (ix > Ld.Nx) return;
    const int npair = (Ld.Ny + 1) / 2;
    for (int k = threadIdx.x; k < npair; k += 256) {
        const int iy = 1 + 2 * k;
        const bool two = iy + 1 <= Ld.Ny;
        const long long o = Ld.at(ix, iy);
        for (int p = 0; p < 3; ++p) {
            double* out = dq + p * Ld.plane + o;
            if (wide && two) *reinterpret_cast<rs_d2*>(out) = rs_d2{value, value};
            else { out[0] = value; if (two) out[1] = value; }
        }
    }
}

}  // namespace gpf
