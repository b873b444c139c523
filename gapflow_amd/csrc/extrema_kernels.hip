// Field extrema of the committed state, each with its cell (entry points in api_extrema.inc): the largest and smallest EOS
// pressure and density, the smallest gap height, the largest |jx / rho| and |jy / rho|, over the interior cells 1..Nx x 1..Ny.
//
// The order on candidates (value, ix, iy), their accumulator, the workgroup fold, the row fold and the stores are
// series_first.hpp's, which states their contract once.  A committed state has no NaN and rho >= 0 (q_is_valid).
// rho = 0 makes |j / rho| inf (NaN for j = 0, which no comparison ever prefers or displaces): plain IEEE, not special-cased.
//
// Three writers, one record (seven doubles, fourteen int32):
//   k_extrema_partial + k_extrema_fold   behind every launch-per-step step, guarded by the device's run state like k_probe_record
//   extrema_record_block                 inside k_small_steps, after commit_step, from the field the workgroup holds in LDS
//                                        (one wave per quantity)
//   extrema_record_wide                  inside k_mid_ensemble, after commit_step, from the workspace planes in device memory
//                                        (the whole block walks the interior once)
// k_extrema_partial runs one 256-thread workgroup per interior row (extrema_row_first, which the slabs' row kernel shares); it
// reads 4 planes (rho, jx, jy, h: 32 B per cell) and stores seven (value, iy) pairs per row; k_extrema_fold folds the Nx rows in
// one workgroup.
#pragma once

#include "series_first.hpp"

namespace gpf {

constexpr int EXTREMA_NQ = 7;       // p_max p_min rho_max rho_min h_min u_max v_max
constexpr unsigned EXTREMA_MIN_MASK = 0b0011010;

struct ExtremaArgs {
    double* val;            // [cap + 1][7]
    int* cell;              // [cap + 1][7][2]: ix, iy in the ghosted index space
    double* row_val;        // [Nx][7]: k_extrema_partial's row results
    int* row_iy;            // [Nx][7]
    long long every, cap;   // recording stride; records a batch may leave (slot cap: gpf_extrema_now's)
};

using ExtAcc = FirstAcc<EXTREMA_NQ, EXTREMA_MIN_MASK>;

__device__ __forceinline__ bool extrema_is_min(int k) { return ExtAcc::is_min(k); }

// One cell's seven candidates
__device__ __forceinline__ void extrema_cell(ExtAcc& a, double p, double rho, double jx, double jy, double h, int cx, int cy) {
    a.take(0, p, cx, cy); a.take(1, p, cx, cy);
    a.take(2, rho, cx, cy); a.take(3, rho, cx, cy);
    a.take(4, h, cx, cy);
    a.take(5, fabs(jx / rho), cx, cy);
    a.take(6, fabs(jy / rho), cx, cy);
}

// The first candidates of interior row ix of the state q over the gap topo, by the row's 256-thread workgroup, valid in thread 0.
// The pair walk is plane_pairs' rule on this function's own code: through plane_pairs the two row kernels took 6 scalar registers
// fewer in every instantiation and a record on a 260 x 522 grid 0.5 us (2 %) longer.
template <int EOS>
__device__ __forceinline__ ExtAcc extrema_row_first(const double* q, const double* topo, const Layout& L, const Phys& P, int wide, int ix, ExtAcc* sm) {
    ExtAcc a;
    a.none();
    const int npair = (L.Ny + 1) / 2;
    for (int k = threadIdx.x; k < npair; k += 256) {
        const int iy = 1 + 2 * k;
        const bool two = iy + 1 <= L.Ny;
        const long long o = L.at(ix, iy);
        series_d2 in[4];
        if (wide) {
#pragma unroll
            for (int p = 0; p < 3; ++p) in[p] = *reinterpret_cast<const series_d2*>(q + p * L.plane + o);
            in[3] = *reinterpret_cast<const series_d2*>(topo + o);
        } else {
            const long long o1 = two ? o + 1 : o;
#pragma unroll
            for (int p = 0; p < 3; ++p) in[p] = series_d2{q[p * L.plane + o], q[p * L.plane + o1]};
            in[3] = series_d2{topo[o], topo[o1]};
        }
        extrema_cell(a, eos_pressure<EOS>(in[0].x, P), in[0].x, in[1].x, in[2].x, in[3].x, ix, iy);
        if (two) extrema_cell(a, eos_pressure<EOS>(in[0].y, P), in[0].y, in[1].y, in[2].y, in[3].y, ix, iy + 1);
    }
    return block_first(a, sm, npair < 256 ? npair : 256);
}

template <int EOS>
__global__ __launch_bounds__(256) void k_extrema_partial(const double* qa, const double* qb, const double* topo, const StepState* st,
                                                         const Layout L, const Phys P, const ExtremaArgs x, int wide, long long expect,
                                                         long long slot) {
    __shared__ ExtAcc sm[4];
    if (series_skip(st, expect, slot, x.cap)) return;
    const int ix = 1 + blockIdx.x;
    const ExtAcc r = extrema_row_first<EOS>(st->parity ? qb : qa, topo, L, P, wide, ix, sm);
    if (threadIdx.x == 0) store_row_first(x.row_val, x.row_iy, ix - 1, r);
}

__global__ __launch_bounds__(256) void k_extrema_fold(const StepState* st, const ExtremaArgs x, int Nx, long long expect, long long slot) {
    __shared__ ExtAcc sm[4];
    if (series_skip(st, expect, slot, x.cap)) return;
    const ExtAcc r = block_first(first_of_rows<ExtAcc>(x.row_val, x.row_iy, Nx), sm, Nx < 256 ? Nx : 256);
    if (threadIdx.x == 0) store_first(x.val, x.cell, slot, r);
}

// The same record from the dense LDS field of k_small_steps (q: planes of nc cells, rows of w; h: the gap plane): the whole
// block (at least seven waves) calls it after the commit of a step whose count is a multiple of the stride, with the slot of
// that step among the batch's recorded steps (a SeriesCursor keeps both; the arguments are fetched from device
// memory once per launch and stay beside it).
// Block-uniform; reads only, and needs no barrier: the committed field is not written again before the commit after next.
// Wave k takes quantity k alone, so that a record costs a fraction of a step: its lanes evaluate the quantity of their
// cells and keep the first, shuffles fold the lanes -- by the same comparison -- and lane 0 stores the value and the cell.
template <int EOS>
__device__ __forceinline__ void extrema_record_block(const ExtremaArgs& x, const double* q, const double* h, int Nx, int Ny, int nc, int w,
                                                     long long slot, const Phys& P) {
    if (slot < 0 || slot >= x.cap) return;
    const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (k >= EXTREMA_NQ) return;                        // wave-uniform
    const int ncell = Nx * Ny;
    const bool want_min = extrema_is_min(k);
    double v = want_min ? __builtin_huge_val() : -__builtin_huge_val();
    int bx = EXTREMA_NO_CELL, by = EXTREMA_NO_CELL;
    for (int t = lane; t < ncell; t += 64) {
        const int ix = 1 + t / Ny, iy = 1 + t % Ny;
        const int c = ix * w + iy;
        double f;
        if (k < 2) f = eos_pressure<EOS>(q[c], P);
        else if (k < 4) f = q[c];
        else if (k == 4) f = h[c];
        else f = fabs(q[(k - 4) * nc + c] / q[c]);      // k 5: jx, k 6: jy
        if (extrema_before(want_min, f, ix, iy, v, bx, by)) { v = f; bx = ix; by = iy; }
    }
    for (int s = 32; s >= 1; s >>= 1) {
        const double ov = __shfl_down(v, s);
        const int ox = __shfl_down(bx, s), oy = __shfl_down(by, s);
        if (extrema_before(want_min, ov, ox, oy, v, bx, by)) { v = ov; bx = ox; by = oy; }
    }
    if (lane == 0) {
        x.val[slot * EXTREMA_NQ + k] = v;
        x.cell[(slot * EXTREMA_NQ + k) * 2] = bx;
        x.cell[(slot * EXTREMA_NQ + k) * 2 + 1] = by;
    }
}

// The same record from the dense workspace planes of k_mid_ensemble (mid_kernel.hip), where a member has up to 126 x 126
// interior cells: one wave per quantity would leave each lane some 250 cells, a division per cell and seven walks, against a
// step whose passes give a thread about 32 cells.  So here the WHOLE block (blockDim.x threads, a multiple of 64, at most 512)
// walks the interior once -- thread t takes the interior cells t, t + blockDim.x, ... in row-major order, a MidCursor of width
// Ny in place of a division per cell --, every thread keeps all seven candidates (extrema_cell: the expressions of
// k_extrema_partial, so p, u_max and v_max carry the same bits), and block_first folds them through `sm` (one ExtAcc per wave).
// The order is total, so the walk's shape does not show in the record.
// Block-uniform; reads only.  The caller has a workgroup barrier between the stores that made q and this call (the planes are
// in device memory: the barrier is their release / acquire), and one between two calls (`sm` is used again).
template <int EOS>
__device__ __forceinline__ void extrema_record_wide(const ExtremaArgs& x, const double* q, const double* h, int Nx, int Ny, int nc, int w,
                                                    long long slot, const Phys& P, ExtAcc* sm) {
    if (slot < 0 || slot >= x.cap) return;              // block-uniform
    const int ncell = Nx * Ny, nt = blockDim.x;
    ExtAcc a;
    a.none();
    MidCursor k(threadIdx.x, nt, Ny);
    for (int t = threadIdx.x; t < ncell; t += nt, k.next()) {
        const int ix = 1 + k.ix, iy = 1 + k.iy;
        const int c = ix * w + iy;
        const double rho = q[c];
        extrema_cell(a, eos_pressure<EOS>(rho, P), rho, q[nc + c], q[2 * nc + c], h[c], ix, iy);
    }
    const ExtAcc r = block_first(a, sm, nt);
    if (threadIdx.x == 0) store_first(x.val, x.cell, slot, r);
}

}  // namespace gpf
