// Deformation series of an elastic handle (entry points in api_elastic_series.inc): what the wall gives way by under the film it
// carries, per recorded step over the interior cells 1..Nx x 1..Ny, with
//   d   the deformation plane the handle holds (el.deformation, what GPF_FIELD_DEFORMATION downloads),
//   p   closures.hpp: film_pressure<EOS> of the committed density -- the p of the film integrals' `load`,
//   h   the deformed gap (plane 0 of the handle's topography):
// four sums times dx dy -- d_sum (the displaced volume), d2_sum (d d: the RMS deflection is sqrt(d2_sum / area)), p_d (p d: twice
// the elastic work of a linear half-space, the factor 1/2 is the user's) and h_sum (the film's volume) -- and d_max, d_min, each
// with its cell (ix, iy) of the ghosted index space.
//
// The two launches per record, the guard, the pair order, the fold tree and the row loop are series_rows.hpp's:
//   k_eldef_partial   one 256-thread workgroup per interior row; reads 3 planes (rho, h, d: 24 B per cell) once; thread 0 stores
//                     the row's four sums and its two extrema with their columns.
//   k_eldef_fold      one workgroup; thread 0 applies dx dy and stores the record.
// The walk is eldef_row_pairs, beside series_rows.hpp: row_pairs and not inside it -- that one fetches the six planes of q and of
// the gap for CellIn and knows no deformation plane, and the kernels built on it keep their registers as long as it stays as it
// is.  Thread t owns the column pairs (1 + 2k, 2 + 2k), k = t, t + 256, ..., the lower column first, one 16-byte load per plane
// where the buffers allow it and two 8-byte loads otherwise; the ghost column an odd Ny reaches is loaded and never handed on.
// The sums go through block_sum and add_rows: who adds what depends on (Nx, Ny) alone.  The products d d and p d are rounded on
// their own (weighted_kernels.hip: the canonicalize between product and sum), so a NumPy restatement of the terms meets the
// device's.  The extrema are ordered by extrema_kernels.hip: extrema_before -- value, then the smaller ix, then the smaller iy --,
// a total order, so the shape of their tree does not matter.  A record is a pure function of (q, gap, deformation): no
// floating-point atomics, the same bits for every stride and for the wide and narrow loads.
#pragma once

#include "series_rows.hpp"
#include "extrema_kernels.hip"

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

// The first candidates for d_max (k = 0) and d_min (k = 1) under extrema_before
struct ElDefExt {
    double v[ELDEF_NEXT];
    int ix[ELDEF_NEXT], iy[ELDEF_NEXT];
    // the candidate every cell comes before
    __device__ __forceinline__ void none() {
        v[0] = -__builtin_huge_val(); v[1] = __builtin_huge_val();
#pragma unroll
        for (int k = 0; k < ELDEF_NEXT; ++k) { ix[k] = EXTREMA_NO_CELL; iy[k] = EXTREMA_NO_CELL; }
    }
    __device__ __forceinline__ void take(int k, double x, int cx, int cy) {
        if (extrema_before(k == 1, x, cx, cy, v[k], ix[k], iy[k])) { v[k] = x; ix[k] = cx; iy[k] = cy; }
    }
};

// The first candidates of the workgroup's 256 threads, valid in thread 0: lanes 32, 16, .. 1 apart, then the four waves.  A
// thread without a cell holds none(), which never displaces a cell.
__device__ __forceinline__ ElDefExt eldef_block_first(ElDefExt a, ElDefExt* sm) {
    for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
        for (int k = 0; k < ELDEF_NEXT; ++k) {
            const double ov = __shfl_down(a.v[k], s);
            const int ox = __shfl_down(a.ix[k], s), oy = __shfl_down(a.iy[k], s);
            a.take(k, ov, ox, oy);
        }
    }
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 4; ++i) {
#pragma unroll
            for (int k = 0; k < ELDEF_NEXT; ++k) a.take(k, sm[i].v[k], sm[i].ix[k], sm[i].iy[k]);
        }
    }
    return a;
}

// The pair walk of row ix in series_rows.hpp: row_pairs' order, over rho, h and d: cell(rho, h, d, iy)
template <class Cell> __device__ __forceinline__ void eldef_row_pairs(const ElDefArgs& f, int ix, Cell cell) {
    const Layout& L = f.L;
    const double* rho = f.st->parity ? f.qb : f.qa;
    const int npair = (L.Ny + 1) / 2;
    for (int k = threadIdx.x; k < npair; k += 256) {
        const int iy = 1 + 2 * k;
        const bool two = iy + 1 <= L.Ny;
        const long long o = L.at(ix, iy);
        series_d2 in[3];
        if (f.wide) {
            in[0] = *reinterpret_cast<const series_d2*>(rho + o);
            in[1] = *reinterpret_cast<const series_d2*>(f.topo + o);
            in[2] = *reinterpret_cast<const series_d2*>(f.d + o);
        } else {
            const long long o1 = two ? o + 1 : o;
            in[0] = series_d2{rho[o], rho[o1]};
            in[1] = series_d2{f.topo[o], f.topo[o1]};
            in[2] = series_d2{f.d[o], f.d[o1]};
        }
        cell(in[0].x, in[1].x, in[2].x, iy);
        if (two) cell(in[0].y, in[1].y, in[2].y, iy + 1);
    }
}

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
    eldef_row_pairs(f, ix, [&](double rho, double h, double d, int iy) {
        const double p = film_pressure<EOS>(rho, P);
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
    const ElDefExt x = eldef_block_first(e, sme);
    if (threadIdx.x == 0) {
        double* out = f.part + (long long)(ix - 1) * ELDEF_NSUM;
#pragma unroll
        for (int k = 0; k < ELDEF_NSUM; ++k) out[k] = r.v[k];
#pragma unroll
        for (int k = 0; k < ELDEF_NEXT; ++k) {
            f.row_val[(long long)(ix - 1) * ELDEF_NEXT + k] = x.v[k];
            f.row_iy[(long long)(ix - 1) * ELDEF_NEXT + k] = x.iy[k];
        }
    }
}

__global__ __launch_bounds__(256) void k_eldef_fold(const ElDefArgs f, long long expect) {
    __shared__ double sm[4][ELDEF_NSUM];
    __shared__ ElDefExt sme[4];
    if (series_skip(f.st, expect, f.slot, f.cap)) return;
    ElDefExt e;
    e.none();
    const ElDefAcc a = add_rows<ELDEF_NSUM>(f.part, 0, f.L.Nx, [&](int row) {
#pragma unroll
        for (int k = 0; k < ELDEF_NEXT; ++k) e.take(k, f.row_val[(long long)row * ELDEF_NEXT + k], row + 1, f.row_iy[(long long)row * ELDEF_NEXT + k]);
    });
    const ElDefAcc r = block_sum(a, sm);
    const ElDefExt x = eldef_block_first(e, sme);
    if (threadIdx.x != 0) return;
    double* out = f.rec + f.slot * ELDEF_NREC;
    int* c = f.cell + f.slot * 2 * ELDEF_NEXT;
    const double dA = f.dx * f.dy;
#pragma unroll
    for (int k = 0; k < ELDEF_NSUM; ++k) out[k] = r.v[k] * dA;
#pragma unroll
    for (int k = 0; k < ELDEF_NEXT; ++k) { out[ELDEF_NSUM + k] = x.v[k]; c[2 * k] = x.ix[k]; c[2 * k + 1] = x.iy[k]; }
}

}  // namespace gpf
