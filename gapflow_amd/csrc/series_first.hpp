// What the recorded series with a maximum or a minimum in them -- field extrema, step changes, an elastic handle's deformation
// series, the domain extrema on x-slabs (extrema_, change_, elastic_series_, slab_series_kernels.hip) -- share on the device: "the
// first candidate (value, ix, iy), with its cell".  The companion of series_rows.hpp, which holds the sums' half.
//
// ONE comparison, extrema_before, orders candidates (value, ix, iy) totally: the better value first, then the smaller ix, then the
// smaller iy.  Every fold -- a thread over its cells, lanes over a wave, waves over a workgroup, rows over the grid -- keeps the
// first of two candidates under that order.  The minimum of a total order does not depend on how the candidates are bracketed, so
// the shape of the reduction tree is free: a record is a pure function of the state (no floating-point atomics, no arrival
// order), and the wide and narrow loads, the row kernels and the one-workgroup kernels agree in every bit.  The values hold no
// NaN (a committed state has none, q_is_valid), or only NaN that no comparison ever prefers or displaces.
//
//   FirstAcc<N, MIN_MASK>   a thread's (a wave's, a row's, a record's) N first candidates; bit k of MIN_MASK: quantity k is a minimum
//   plane_pairs<NP>         the pair walk of an interior row over NP planes, in series_rows.hpp: row_pairs' order
//   block_first             the workgroup's first candidates, valid in thread 0
//   store_row_first         a row's (value, iy) into the row scratch [nrow][N]; first_of_rows folds that scratch in the second launch
//   store_first             a record's (value, ix, iy) into [slot][N] and [slot][N][2]
// A new series with extrema is a FirstAcc, a cell functor for plane_pairs and the epilogues of its two kernels.
//
// The comparison and FirstAcc compile for the host on their own (tests/test_series_first_hostcheck.py folds candidate sets
// with them in every bracketing); the rest is device code.
#pragma once

#if defined(__HIPCC__)
#include "series_rows.hpp"
#define GPF_FIRST_FN __device__ __forceinline__
#else
#define GPF_FIRST_FN inline
#endif

namespace gpf {

constexpr int EXTREMA_NO_CELL = 0x7fffffff;

// THE comparison: does candidate a come before candidate b?  A total order on (value, ix, iy) for values without NaN.
GPF_FIRST_FN bool extrema_before(bool want_min, double a, int ax, int ay, double b, int bx, int by) {
    if (a != b) return want_min ? a < b : a > b;
    return ax != bx ? ax < bx : ay < by;
}

template <int N, unsigned MIN_MASK> struct FirstAcc {
    static constexpr int n = N;
    double v[N];
    int ix[N], iy[N];
    static constexpr bool is_min(int k) { return (MIN_MASK >> k) & 1u; }
    // the candidate every cell comes before
    GPF_FIRST_FN void none() {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            v[k] = is_min(k) ? __builtin_huge_val() : -__builtin_huge_val();
            ix[k] = EXTREMA_NO_CELL; iy[k] = EXTREMA_NO_CELL;
        }
    }
    GPF_FIRST_FN void take(int k, double x, int cx, int cy) {
        if (extrema_before(is_min(k), x, cx, cy, v[k], ix[k], iy[k])) { v[k] = x; ix[k] = cx; iy[k] = cy; }
    }
    GPF_FIRST_FN void merge(const FirstAcc& o) {
#pragma unroll
        for (int k = 0; k < N; ++k) take(k, o.v[k], o.ix[k], o.iy[k]);
    }
};

#if defined(__HIPCC__)

// The pair walk of interior row ix over the NP planes `planes` of layout L, by a 256-thread workgroup: thread t owns the column
// pairs (1 + 2k, 2 + 2k) for k = t, t + 256, ... and hands cell(x, iy) the NP values x of its cells in that order, the lower
// column first.  A pair is fetched with one 16-byte load per plane if `wide` (api_series.inc: series_wide_ok) and with two
// 8-byte loads otherwise; the column Ny + 1 that the last pair of an odd Ny reaches is the row's ghost cell: it is loaded and
// never handed on.
template <int NP, class Cell>
__device__ __forceinline__ void plane_pairs(const double* const (&planes)[NP], const Layout& L, int wide, int ix, Cell cell) {
    const int npair = (L.Ny + 1) / 2;
    for (int k = threadIdx.x; k < npair; k += 256) {
        const int iy = 1 + 2 * k;
        const bool two = iy + 1 <= L.Ny;
        const long long o = L.at(ix, iy);
        series_d2 in[NP];
        if (wide) {
#pragma unroll
            for (int p = 0; p < NP; ++p) in[p] = *reinterpret_cast<const series_d2*>(planes[p] + o);
        } else {
            const long long o1 = two ? o + 1 : o;
#pragma unroll
            for (int p = 0; p < NP; ++p) in[p] = series_d2{planes[p][o], planes[p][o1]};
        }
        double x[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) x[p] = in[p].x;
        cell(x, iy);
        if (two) {
#pragma unroll
            for (int p = 0; p < NP; ++p) x[p] = in[p].y;
            cell(x, iy + 1);
        }
    }
}

// The first candidates of all threads of the workgroup (blockDim.x a multiple of 64, at most 512), valid in thread 0.  Only
// threads 0 .. nactive - 1 (nactive >= 1, block-uniform) hold candidates: the waves among them fold their lanes 32, 16, .. 1
// apart, then thread 0 folds those waves; a wave wholly beyond nactive holds nothing and does nothing.  A thread among them
// without a cell holds none(), which never displaces a cell.  `sm`, one entry per wave, is written by lane 0 of every such wave
// and read by thread 0 only: a caller that uses it again puts a barrier in between.
template <int N, unsigned M> __device__ __forceinline__ FirstAcc<N, M> block_first(FirstAcc<N, M> a, FirstAcc<N, M>* sm, int nactive) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if ((w << 6) < nactive) {                           // wave-uniform
        for (int s = 32; s >= 1; s >>= 1) {
            FirstAcc<N, M> o;
#pragma unroll
            for (int k = 0; k < N; ++k) { o.v[k] = __shfl_down(a.v[k], s); o.ix[k] = __shfl_down(a.ix[k], s); o.iy[k] = __shfl_down(a.iy[k], s); }
            a.merge(o);
        }
        if (lane == 0) sm[w] = a;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int nw = (nactive + 63) >> 6;
        for (int i = 1; i < nw; ++i) a.merge(sm[i]);
    }
    return a;
}

// Thread 0 of a row's workgroup: the row's (value, iy) into the scratch [nrow][N] (the row is the ix)
template <int N, unsigned M> __device__ __forceinline__ void store_row_first(double* row_val, int* row_iy, int row, const FirstAcc<N, M>& r) {
    double* v = row_val + (long long)row * N;
    int* c = row_iy + (long long)row * N;
#pragma unroll
    for (int k = 0; k < N; ++k) { v[k] = r.v[k]; c[k] = r.iy[k]; }
}

// A fold thread's first candidates of that scratch: thread t takes rows t, t + 256, ..., row `row` being ix = row + 1
template <class Acc> __device__ __forceinline__ Acc first_of_rows(const double* row_val, const int* row_iy, int nrow) {
    Acc a;
    a.none();
    for (int row = threadIdx.x; row < nrow; row += 256) {
        const double* v = row_val + (long long)row * Acc::n;
        const int* c = row_iy + (long long)row * Acc::n;
#pragma unroll
        for (int k = 0; k < Acc::n; ++k) a.take(k, v[k], row + 1, c[k]);
    }
    return a;
}

// A record's candidates: the values into val[slot * per + k] (`per` doubles per record, the N values leading those `val` points
// at), the cells into cell[slot][N][2] as (ix, iy)
template <int N, unsigned M>
__device__ __forceinline__ void store_first(double* val, int* cell, long long slot, const FirstAcc<N, M>& r, int per = N) {
    double* v = val + slot * per;
    int* c = cell + slot * 2 * N;
#pragma unroll
    for (int k = 0; k < N; ++k) { v[k] = r.v[k]; c[2 * k] = r.ix[k]; c[2 * k + 1] = r.iy[k]; }
}

#endif  // __HIPCC__

}  // namespace gpf
