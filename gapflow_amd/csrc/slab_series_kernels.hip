// Domain series on x-slabs (entry points in api_slab_series.inc): the film integrals and the field extrema of the WHOLE domain,
// recorded by every rank of a slab run, bit for bit the record the undivided handle writes for the same state.
//
// Both series are row-reduced (series_rows.hpp): one workgroup reduces an interior row to a vector, one workgroup folds the
// rows' vectors.  Slabs are cut along rows, so a row's vector is computed where the row lives and only the fold has to see all of
// them:
//   k_slab_film_partial     k_film_partial's walk (row_pairs, film_cell<EOS>, block_sum, unchanged) over this rank's rows; the cell
//                           centre x is spelled from the GLOBAL row, ((double)(ix + row0) - 0.5) * dx -- for the global row
//                           ix + row0 the very expression k_film_partial evaluates.  The row's [FILM_NV] goes into this rank's
//                           message at local row ix - 1.  The y-sections' columns are global already.
//   k_slab_extrema_partial  k_extrema_partial's row (extrema_kernels.hip: extrema_row_first); the row's seven (value, iy) go into the
//                           message behind the film vector, iy as a double (exact), so that ONE all-gather of doubles carries both
//                           series.
//   (the host gathers the messages: gathered[world][max_nx][SLAB_SERIES_W], slab_rows.hpp)
//   k_slab_film_fold        one workgroup on every rank: thread t adds the vectors of the global rows t, t + 256, ... in that order
//                           to +0.0 (add_rows' loop, each row found through slab_rows.hpp), block_sum, then k_film_fold's epilogue:
//                           dx dy on the nine sums, the gathered row of global section sx[k] times dy, the folded section slots
//                           times dx.  The same expression tree over the same operands as fold_rows + k_film_fold: the same bits.
//   k_slab_extrema_fold     k_extrema_fold's fold with ix = g + 1, the global row in the ghosted index space, on a row loop of its
//                           own (the rows are found through slab_rows.hpp, the columns read back from doubles); block_first and
//                           store_first are series_first.hpp's.  The order on (value, ix, iy) is total, so the bracket is free.
// Every rank folds the same gathered buffer in the same order, so every rank holds the same record, as it holds the same dt.
// A record is a pure function of the domain's state: no floating-point atomics, no arrival order.  Padding rows of the gathered
// buffer (local rows >= a rank's own count) are never read.  All four kernels are guarded by series_skip like every recorder; the
// folds also note the simulated time of the record, which a slab's host has no per-step log to take it from.
// No slip-length variant: SlabProblem never uploads a slip-length plane, and gpf_slab_series_set refuses a handle that holds one.
#pragma once

#include "extrema_kernels.hip"
#include "integral_kernels.hip"
#include "slab_rows.hpp"

namespace gpf {

constexpr int SLAB_SERIES_EXT = FILM_NV;                        // a message row: the film vector, seven values, seven iy
constexpr int SLAB_SERIES_W = FILM_NV + 2 * EXTREMA_NQ;

// The leading part by name is what row_pairs and series_row_args expect (series_rows.hpp, api_series.inc)
struct SlabFilmArgs {
    const double *qa, *qb, *topo, *Ls;
    const StepState* st;
    double* msg;            // partial: this rank's message [max_nx][SLAB_SERIES_W]
    const double* gathered; // fold: [nranks][max_nx][SLAB_SERIES_W]
    double* rec;            // [cap + 1][9 + nsx + nsy], as FilmArgs::rec
    double* time;           // [cap + 1]: simulated time of each record
    Layout L;
    double dx, dy;
    int nsx, nsy;
    int sx[FILM_MAX_SECTIONS], sy[FILM_MAX_SECTIONS];       // GLOBAL interior rows / columns of the sections
    int wide;
    int row0, nx_global, nranks;    // global rows below this slab's first; the domain's rows; the ranks of the cut
    long long slot, cap;
};

struct SlabExtremaArgs {
    const double *qa, *qb, *topo;
    const StepState* st;
    double* msg;
    const double* gathered;
    double* time;           // [cap + 1]
    ExtremaArgs x;          // val, cell, cap (the row scratch is the message)
    Layout L;
    int wide;
    int nx_global, nranks;
    long long slot;
};

template <int EOS>
__global__ __launch_bounds__(256) void k_slab_film_partial(const SlabFilmArgs f, const Phys P, long long expect) {
    __shared__ double sm[4][FILM_NV];
    if (series_skip(f.st, expect, f.slot, f.cap)) return;
    const int ix = 1 + blockIdx.x;
    const double x = ((double)(ix + f.row0) - 0.5) * f.dx;
    FilmAcc a;
    a.zero();
    row_pairs<FilmPlanes<false>>(f, nullptr, ix, [&](const CellIn& c, double, int iy, double y) { film_cell<EOS>(a, f, P, c, x, y, iy); });
    const FilmAcc r = block_sum(a, sm);
    if (threadIdx.x == 0) {
        double* out = f.msg + (long long)(ix - 1) * SLAB_SERIES_W;
#pragma unroll
        for (int k = 0; k < FILM_NV; ++k) out[k] = r.v[k];
    }
}

__global__ __launch_bounds__(256) void k_slab_film_fold(const SlabFilmArgs f, long long expect) {
    __shared__ double sm[4][FILM_NV];
    if (series_skip(f.st, expect, f.slot, f.cap)) return;
    FilmAcc a;
    a.zero();
    for (int g = threadIdx.x; g < f.nx_global; g += 256) {
        const double* in = f.gathered + slab_gathered_row(g, f.nx_global, f.nranks) * SLAB_SERIES_W;
#pragma unroll
        for (int k = 0; k < FILM_NV; ++k) a.v[k] += in[k];
    }
    const FilmAcc r = block_sum(a, sm);
    if (threadIdx.x != 0) return;
    const int nrec = FILM_NSUM + f.nsx + f.nsy;
    double* out = f.rec + f.slot * nrec;
    const double dA = f.dx * f.dy;
#pragma unroll
    for (int k = 0; k < FILM_NSUM; ++k) out[k] = r.v[k] * dA;
    for (int k = 0; k < f.nsx; ++k)
        out[FILM_NSUM + k] = f.gathered[slab_gathered_row(f.sx[k] - 1, f.nx_global, f.nranks) * SLAB_SERIES_W + FILM_NSUM] * f.dy;
#pragma unroll
    for (int k = 0; k < FILM_MAX_SECTIONS; ++k)
        if (k < f.nsy) out[FILM_NSUM + f.nsx + k] = r.v[FILM_NSUM + 1 + k] * f.dx;
    f.time[f.slot] = f.st->simtime;
}

template <int EOS>
__global__ __launch_bounds__(256) void k_slab_extrema_partial(const SlabExtremaArgs e, const Phys P, long long expect) {
    __shared__ ExtAcc sm[4];
    if (series_skip(e.st, expect, e.slot, e.x.cap)) return;
    const int ix = 1 + blockIdx.x;
    const ExtAcc r = extrema_row_first<EOS>(e.st->parity ? e.qb : e.qa, e.topo, e.L, P, e.wide, ix, sm);
    if (threadIdx.x == 0) {
        double* out = e.msg + (long long)(ix - 1) * SLAB_SERIES_W + SLAB_SERIES_EXT;
#pragma unroll
        for (int k = 0; k < EXTREMA_NQ; ++k) { out[k] = r.v[k]; out[EXTREMA_NQ + k] = (double)r.iy[k]; }
    }
}

__global__ __launch_bounds__(256) void k_slab_extrema_fold(const SlabExtremaArgs e, long long expect) {
    __shared__ ExtAcc sm[4];
    if (series_skip(e.st, expect, e.slot, e.x.cap)) return;
    ExtAcc a;
    a.none();
    for (int g = threadIdx.x; g < e.nx_global; g += 256) {
        const double* in = e.gathered + slab_gathered_row(g, e.nx_global, e.nranks) * SLAB_SERIES_W + SLAB_SERIES_EXT;
#pragma unroll
        for (int k = 0; k < EXTREMA_NQ; ++k) a.take(k, in[k], g + 1, (int)in[EXTREMA_NQ + k]);
    }
    const ExtAcc r = block_first(a, sm, e.nx_global < 256 ? e.nx_global : 256);
    if (threadIdx.x == 0) {
        store_first(e.x.val, e.x.cell, e.slot, r);
        e.time[e.slot] = e.st->simtime;
    }
}

}  // namespace gpf
