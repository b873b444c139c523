// Step-change series (entry points in api_changes.inc): how far the committed step n moved each conserved field, over the interior
// cells 1..Nx x 1..Ny, with d = q^n - q^(n-1) per field (rho, jx, jy):
//   d2_*     sum of d d          times dx dy
//   q2_*     sum of q^n q^n      times dx dy   (the relative L2 change is sqrt(d2 / q2), its rate that over dt)
//   dmass    sum of d_rho h      times dx dy   (h: plane 0 of the gap the handle holds)
//   dmax_*   max |d|, each with its cell (ix, iy) of the ghosted index space
//   dt       StepState::dt_last, the step size of that step
// q^n is q[parity]; q^(n-1) is the OTHER buffer: k_step2 reads one buffer and writes the other, k_small_steps leaves the state
// before its last committed step there on exit, a checkpoint carries it.  The host knows when that holds (prev_state_valid) and
// launches these kernels only then.  d of neighbouring states is a difference of nearly equal numbers and therefore (almost
// always) exact, which is why dmass resolves the mass defect of one step where the difference of two global sums does not.
//
// The two launches per record, the guard, the fold tree and the row loop of the sums are series_rows.hpp's; the maxima -- their
// order, accumulator, folds and stores -- are series_first.hpp's.  The pair walk is plane_pairs' rule on the kernel's
// own code: through plane_pairs its seven planes cost k_change_partial 9 VGPRs (66 -> 75) and a wave per SIMD (7 -> 6).
//   k_change_partial   one 256-thread workgroup per interior row; reads 7 planes (three of each buffer and h: 56 B per cell) once;
//                      thread 0 stores the row's seven sums and its three maxima with their columns.
//   k_change_fold      one workgroup; thread 0 applies dx dy, copies dt_last and stores the record.
// The sums go through block_sum and fold_rows: who adds what depends on (Nx, Ny) alone.  Every product (d d, q q, d_rho h) is
// rounded on its own (elastic_series_kernels.hip: the canonicalize between product and sum), so a NumPy restatement of the terms
// meets the device's.  A record is a pure function of (q^n, q^(n-1), h, dt_last): no floating-point atomics, no arrival order,
// the same bits for every stride and for the wide and narrow loads.
#pragma once

#include "series_first.hpp"

namespace gpf {

constexpr int CHANGE_NSUM = 7;          // d2_rho d2_jx d2_jy q2_rho q2_jx q2_jy dmass
constexpr int CHANGE_NMAX = 3;          // dmax_rho dmax_jx dmax_jy
constexpr int CHANGE_NREC = CHANGE_NSUM + CHANGE_NMAX + 1;      // ... and dt

struct ChangeArgs {
    const double *qa, *qb, *topo;
    const StepState* st;
    double* part;           // [Nx][CHANGE_NSUM]
    double* row_val;        // [Nx][3]: the row's maxima
    int* row_iy;            // [Nx][3]: their columns
    double* rec;            // [cap + 1][CHANGE_NREC]
    int* cell;              // [cap + 1][3][2]: (ix, iy) of dmax_rho, dmax_jx, dmax_jy
    Layout L;
    double dx, dy;
    int wide;               // 16-byte pair loads are aligned
    long long slot, cap;    // record to write; slots the buffer holds
};

using ChangeAcc = RowAcc<CHANGE_NSUM>;
using ChangeExt = FirstAcc<CHANGE_NMAX, 0>;     // three maxima (|d| >= 0)

// One cell's terms: qn, qo the three fields of the new and of the previous state, h the gap
__device__ __forceinline__ void change_cell(ChangeAcc& a, ChangeExt& e, const double qn[3], const double qo[3], double h, int ix, int iy) {
    double d[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) d[p] = qn[p] - qo[p];
    {
#pragma clang fp contract(off)
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            a.v[p] += __builtin_canonicalize(d[p] * d[p]);
            a.v[3 + p] += __builtin_canonicalize(qn[p] * qn[p]);
        }
        a.v[6] += __builtin_canonicalize(d[0] * h);
    }
#pragma unroll
    for (int p = 0; p < 3; ++p) e.take(p, fabs(d[p]), ix, iy);
}

__global__ __launch_bounds__(256) void k_change_partial(const ChangeArgs f, long long expect) {
    __shared__ double sm[4][CHANGE_NSUM];
    __shared__ ChangeExt sme[4];
    if (series_skip(f.st, expect, f.slot, f.cap)) return;
    const Layout& L = f.L;
    const int ix = 1 + blockIdx.x;
    if (ix > L.Nx) return;
    const double* qn = f.st->parity ? f.qb : f.qa;      // q^n
    const double* qo = f.st->parity ? f.qa : f.qb;      // q^(n-1)
    ChangeAcc a;
    a.zero();
    ChangeExt e;
    e.none();
    const int npair = (L.Ny + 1) / 2;
    for (int k = threadIdx.x; k < npair; k += 256) {
        const int iy = 1 + 2 * k;
        const bool two = iy + 1 <= L.Ny;
        const long long o = L.at(ix, iy);
        series_d2 n[3], b[3], h;
        if (f.wide) {
#pragma unroll
            for (int p = 0; p < 3; ++p) n[p] = *reinterpret_cast<const series_d2*>(qn + p * L.plane + o);
#pragma unroll
            for (int p = 0; p < 3; ++p) b[p] = *reinterpret_cast<const series_d2*>(qo + p * L.plane + o);
            h = *reinterpret_cast<const series_d2*>(f.topo + o);
        } else {
            const long long o1 = two ? o + 1 : o;
#pragma unroll
            for (int p = 0; p < 3; ++p) n[p] = series_d2{qn[p * L.plane + o], qn[p * L.plane + o1]};
#pragma unroll
            for (int p = 0; p < 3; ++p) b[p] = series_d2{qo[p * L.plane + o], qo[p * L.plane + o1]};
            h = series_d2{f.topo[o], f.topo[o1]};
        }
        {
            const double cn[3] = {n[0].x, n[1].x, n[2].x}, co[3] = {b[0].x, b[1].x, b[2].x};
            change_cell(a, e, cn, co, h.x, ix, iy);
        }
        if (two) {
            const double cn[3] = {n[0].y, n[1].y, n[2].y}, co[3] = {b[0].y, b[1].y, b[2].y};
            change_cell(a, e, cn, co, h.y, ix, iy + 1);
        }
    }
    const ChangeAcc r = block_sum(a, sm);
    const ChangeExt x = block_first(e, sme, 256);
    if (threadIdx.x == 0) {
        double* out = f.part + (long long)(ix - 1) * CHANGE_NSUM;
#pragma unroll
        for (int k = 0; k < CHANGE_NSUM; ++k) out[k] = r.v[k];
        store_row_first(f.row_val, f.row_iy, ix - 1, x);
    }
}

__global__ __launch_bounds__(256) void k_change_fold(const ChangeArgs f, long long expect) {
    __shared__ double sm[4][CHANGE_NSUM];
    __shared__ ChangeExt sme[4];
    if (series_skip(f.st, expect, f.slot, f.cap)) return;
    const int Nx = f.L.Nx;
    const ChangeAcc r = fold_rows<CHANGE_NSUM>(f.part, 0, Nx, sm);
    const ChangeExt x = block_first(first_of_rows<ChangeExt>(f.row_val, f.row_iy, Nx), sme, 256);
    if (threadIdx.x != 0) return;
    double* out = f.rec + f.slot * CHANGE_NREC;
    const double dA = f.dx * f.dy;
#pragma unroll
    for (int k = 0; k < CHANGE_NSUM; ++k) out[k] = r.v[k] * dA;
    store_first(f.rec + CHANGE_NSUM, f.cell, f.slot, x, CHANGE_NREC);
    out[CHANGE_NREC - 1] = f.st->dt_last;
}

}  // namespace gpf
