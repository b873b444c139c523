// Deformation series of an elastic handle (entry points in api_elastic_series.inc): what the wall gives way by under the film it
// carries, per recorded step over the interior cells 1..Nx x 1..Ny, with
//   d   the deformation plane the handle holds (el.deformation, what GPF_FIELD_DEFORMATION downloads),
//   p   closures.hpp: film_pressure<EOS> of the committed density -- the p of the film integrals' `load`,
//   h   the deformed gap (plane 0 of the handle's topography):
// four sums times dx dy -- d_sum (the displaced volume), d2_sum (d d: the RMS deflection is sqrt(d2_sum / area)), p_d (p d: twice
// the elastic work of a linear half-space, the factor 1/2 is the user's) and h_sum (the film's volume) -- and d_max, d_min, each
// with its cell (ix, iy) of the ghosted index space.
//
// The two launches per record, the guard, the fold tree and the row loop of the sums are series_rows.hpp's; the pair walk
// (plane_pairs over rho, h and d, row_pairs' order) and the two extrema -- their order, accumulator, folds and stores -- are
// series_first.hpp's:
//   k_eldef_partial   one 256-thread workgroup per interior row; reads 3 planes (rho, h, d: 24 B per cell) once; thread 0 stores
//                     the row's four sums and its two extrema with their columns.
//   k_eldef_fold      one workgroup; thread 0 applies dx dy and stores the record.
// The sums go through block_sum and fold_rows: who adds what depends on (Nx, Ny) alone.  The products d d and p d are rounded on
// their own (weighted_kernels.hip: the canonicalize between product and sum), so a NumPy restatement of the terms meets the
// device's.  A record is a pure function of (q, gap, deformation): no floating-point atomics, the same bits for every stride
// and for the wide and narrow loads.
#pragma once

#include "series_first.hpp"

namespace gpf {

constexpr int ELDEF_NSUM = 4;           // d_sum d2_sum p_d h_sum
constexpr int ELDEF_NEXT = 2;           // d_max d_min
constexpr int ELDEF_NREC = ELDEF_NSUM + ELDEF_NEXT;

struct ElDefArgs {
    const double *qa, *qb, *topo, *d;
    const StepState* st;
    double* part;           // [Nx][ELDEF_NSUM]
    double* row_val;        // [Nx][2]: the row's d_max, d_min
    int* row_iy;            // [Nx][2]: their columns
    double* rec;            // [cap + 1][ELDEF_NREC]: the four sums, d_max, d_min
    int* cell;              // [cap + 1][2][2]: (ix, iy) of d_max, of d_min
    Layout L;
    double dx, dy;
    int wide;               // 16-byte pair loads are aligned
    long long slot, cap;    // record to write; slots the buffer holds
};

using ElDefAcc = RowAcc<ELDEF_NSUM>;
using ElDefExt = FirstAcc<ELDEF_NEXT, 0b10>;    // d_max (k = 0), d_min (k = 1)

template <int EOS>
__global__ __launch_bounds__(256) void k_eldef_partial(const ElDefArgs f, const Phys P, long long expect) {
    __shared__ double sm[4][ELDEF_NSUM];
    __shared__ ElDefExt sme[4];
    if (series_skip(f.st, expect, f.slot, f.cap)) return;
    const int ix = 1 + blockIdx.x;
    if (ix > f.L.Nx) return;
    ElDefAcc a;
    a.zero();
    ElDefExt e;
    e.none();
    const double* const planes[3] = {f.st->parity ? f.qb : f.qa, f.topo, f.d};      // rho, h, d
    plane_pairs<3>(planes, f.L, f.wide, ix, [&](const double (&x)[3], int iy) {
        const double h = x[1], d = x[2];
        const double p = film_pressure<EOS>(x[0], P);
        a.v[0] += d;
        {
#pragma clang fp contract(off)
            a.v[1] += __builtin_canonicalize(d * d);
            a.v[2] += __builtin_canonicalize(p * d);
        }
        a.v[3] += h;
        e.take(0, d, ix, iy);
        e.take(1, d, ix, iy);
    });
    const ElDefAcc r = block_sum(a, sm);
    const ElDefExt x = block_first(e, sme, 256);
    if (threadIdx.x == 0) {
        double* out = f.part + (long long)(ix - 1) * ELDEF_NSUM;
#pragma unroll
        for (int k = 0; k < ELDEF_NSUM; ++k) out[k] = r.v[k];
        store_row_first(f.row_val, f.row_iy, ix - 1, x);
    }
}

__global__ __launch_bounds__(256) void k_eldef_fold(const ElDefArgs f, long long expect) {
    __shared__ double sm[4][ELDEF_NSUM];
    __shared__ ElDefExt sme[4];
    if (series_skip(f.st, expect, f.slot, f.cap)) return;
    const int Nx = f.L.Nx;
    const ElDefAcc r = fold_rows<ELDEF_NSUM>(f.part, 0, Nx, sm);
    const ElDefExt x = block_first(first_of_rows<ElDefExt>(f.row_val, f.row_iy, Nx), sme, 256);
    if (threadIdx.x != 0) return;
    double* out = f.rec + f.slot * ELDEF_NREC;
    const double dA = f.dx * f.dy;
#pragma unroll
    for (int k = 0; k < ELDEF_NSUM; ++k) out[k] = r.v[k] * dA;
    store_first(f.rec + ELDEF_NSUM, f.cell, f.slot, x, ELDEF_NREC);
}

}  // namespace gpf
