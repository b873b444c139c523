// What the row-reduced series -- film integrals, weighted integrals, regions (integral_, weighted_, region_kernels.hip) and, for
// the guard and the cursor, the extrema (extrema_kernels.hip) -- share on the device; the companion of api_series.inc.  Each of
// them records the committed state with two launches, both guarded by the device's run state (series_skip) like k_probe_record:
//   k_*_partial   one 256-thread workgroup per interior row ix (and per weight / region on blockIdx.y).  row_pairs: thread t owns
//                 the column pairs (1 + 2k, 2 + 2k) for k = t, t + 256, ... and hands their cells to the series' cell functor in
//                 that order, the lower column first.  A pair is fetched with one 16-byte load per plane where the buffers allow it
//                 (Layout::at puts column 1 at element off + 1 = 16 of a row whose pitch is a multiple of 16 doubles; the host
//                 checks this, the parity of `plane` and the base pointers: api_series.inc, series_wide_ok) and with two 8-byte
//                 loads otherwise; the column Ny + 1 that the last pair of an odd Ny reaches is the row's ghost cell: it is loaded
//                 and never handed on.  Which planes a series reads is a compile-time choice (RowPlanes).
//   k_*_fold      one workgroup (per weight / region).  add_rows: thread t adds the rows' vectors t, t + 256, ... in order.
// Sums are folded by block_sum in both: the 256 register sets in a fixed tree, shuffles 32, 16, .. 1 apart inside a wave, then
// waves 0, 1, 2, 3 added in order to +0.0, valid in thread 0.  Who adds what, and in which order, depends on (Nx, Ny) alone: a
// record is a pure function of the state -- no floating-point atomics, no arrival order, no ticket.  The series' bit-for-bit
// claims (a plane of ones reproduces the film integrals, a region equals the weighted integral of its mask, film_record_block
// replays the two launches) hold because this walk, this tree and this row loop are the only ones.
// The series that keep a maximum or a minimum with its cell walk their rows the same way over their own planes and fold their
// first candidates through the companion header, series_first.hpp.
// A new row-reduced series is a plane selection, a cell functor and the epilogues of its two kernels.
#pragma once

#include "device_types.hpp"

namespace gpf {

typedef double series_d2 __attribute__((ext_vector_type(2)));

// Uniform guard of every recording kernel: the step did not run or was rolled back, or the slot lies outside the buffer
__device__ __forceinline__ bool series_skip(const StepState* st, long long expect, long long slot, long long cap) {
    if (st->step != expect || st->invalid != 0) return true;
    return slot < 0 || slot > cap;
}

// The planes a walk reads: rho, jx, jy of q[parity] and h, hx, hy of the gap always; the slip-length plane; a weight plane.
// A cell's Ls that is not read is 0.0, its weight 1.0.
template <bool HAS_LS, bool HAS_W> struct RowPlanes {
    static constexpr bool has_ls = HAS_LS, has_w = HAS_W;
};
template <bool HAS_LS> using FilmPlanes = RowPlanes<HAS_LS, false>;         // the film integrals' and the regions'
template <bool HAS_LS> using WFilmPlanes = RowPlanes<HAS_LS, true>;         // those and `wp`

// The pair walk of row ix: cell(c, w, iy, y) for the thread's cells in order, y the cell centre as film_record_block spells it
// too.  `f`: FilmArgs, WFilmArgs or RegionArgs -- qa, qb, topo, Ls, st, L, dy and wide are read (api_series.inc: series_row_args
// fills them); each keeps its own layout, on which its kernels' register use depends.
template <class Planes, class Args, class Cell>
__device__ __forceinline__ void row_pairs(const Args& f, const double* wp, int ix, Cell cell) {
    const Layout& L = f.L;
    const double* q = f.st->parity ? f.qb : f.qa;
    const int npair = (L.Ny + 1) / 2;
    for (int k = threadIdx.x; k < npair; k += 256) {
        const int iy = 1 + 2 * k;
        const bool two = iy + 1 <= L.Ny;
        const long long o = L.at(ix, iy);
        series_d2 in[8];
        in[6] = series_d2{0.0, 0.0};
        in[7] = series_d2{1.0, 1.0};
        if (f.wide) {
#pragma unroll
            for (int p = 0; p < 3; ++p) in[p] = *reinterpret_cast<const series_d2*>(q + p * L.plane + o);
#pragma unroll
            for (int p = 0; p < 3; ++p) in[3 + p] = *reinterpret_cast<const series_d2*>(f.topo + p * L.plane + o);
            if (Planes::has_ls) in[6] = *reinterpret_cast<const series_d2*>(f.Ls + o);
            if (Planes::has_w) in[7] = *reinterpret_cast<const series_d2*>(wp + o);
        } else {
            const long long o1 = two ? o + 1 : o;
#pragma unroll
            for (int p = 0; p < 3; ++p) in[p] = series_d2{q[p * L.plane + o], q[p * L.plane + o1]};
#pragma unroll
            for (int p = 0; p < 3; ++p) in[3 + p] = series_d2{f.topo[p * L.plane + o], f.topo[p * L.plane + o1]};
            if (Planes::has_ls) in[6] = series_d2{f.Ls[o], f.Ls[o1]};
            if (Planes::has_w) in[7] = series_d2{wp[o], wp[o1]};
        }
        CellIn c;
        c.rho = in[0].x; c.jx = in[1].x; c.jy = in[2].x; c.h = in[3].x; c.hx = in[4].x; c.hy = in[5].x; c.Ls = in[6].x;
        cell(c, in[7].x, iy, ((double)iy - 0.5) * f.dy);
        if (two) {
            c.rho = in[0].y; c.jx = in[1].y; c.jy = in[2].y; c.h = in[3].y; c.hx = in[4].y; c.hy = in[5].y; c.Ls = in[6].y;
            cell(c, in[7].y, iy + 1, ((double)iy + 0.5) * f.dy);
        }
    }
}

// The densities around a cell whose own is CellIn::rho: rows ix - 1, ix + 1 at its column, columns iy - 1, iy + 1 of its row
struct RhoCross {
    double xm, xp, ym, yp;
};

// row_pairs' companion for a series whose cell needs the 5-point stencil of the density (thinning_series_kernels.hip: grad p):
// the same pairs in the same order from the same loads of the row's own planes, and cell(c, s, iy) with s the four
// neighbours' densities, ghost cells among them.  Of rows ix - 1 and ix + 1 (the ghost rows 0 and Nx + 1 for the first and the
// last interior row) the pair's two columns are fetched as the own row's are -- the pitch is even where `wide` holds, so they
// are aligned alike --; the pair's neighbours inside the row are the column iy - 1 before it (the ghost 0 for the first pair) and
// the column iy + 2 behind it.  Two rules for an odd Ny: the upper column of the last pair is the row's ghost Ny + 1, which is
// the lower cell's neighbour and is never handed on as a cell; and iy + 2 = Ny + 2 then lies outside the row and is not read.
// No weight plane.  `f`: as row_pairs'.
template <class Planes, class Args, class Cell>
__device__ __forceinline__ void row_pairs_cross(const Args& f, int ix, Cell cell) {
    const Layout& L = f.L;
    const double* q = f.st->parity ? f.qb : f.qa;
    const int npair = (L.Ny + 1) / 2;
    for (int k = threadIdx.x; k < npair; k += 256) {
        const int iy = 1 + 2 * k;
        const bool two = iy + 1 <= L.Ny;
        const long long o = L.at(ix, iy), om = o - L.pitch, op = o + L.pitch;
        series_d2 in[7], rm, rp;
        in[6] = series_d2{0.0, 0.0};
        if (f.wide) {
#pragma unroll
            for (int p = 0; p < 3; ++p) in[p] = *reinterpret_cast<const series_d2*>(q + p * L.plane + o);
#pragma unroll
            for (int p = 0; p < 3; ++p) in[3 + p] = *reinterpret_cast<const series_d2*>(f.topo + p * L.plane + o);
            if (Planes::has_ls) in[6] = *reinterpret_cast<const series_d2*>(f.Ls + o);
            rm = *reinterpret_cast<const series_d2*>(q + om);
            rp = *reinterpret_cast<const series_d2*>(q + op);
        } else {
            const long long o1 = two ? o + 1 : o;
            in[0] = series_d2{q[o], q[o + 1]};              // (the ghost Ny + 1 of an odd Ny: the lower cell's neighbour)
#pragma unroll
            for (int p = 1; p < 3; ++p) in[p] = series_d2{q[p * L.plane + o], q[p * L.plane + o1]};
#pragma unroll
            for (int p = 0; p < 3; ++p) in[3 + p] = series_d2{f.topo[p * L.plane + o], f.topo[p * L.plane + o1]};
            if (Planes::has_ls) in[6] = series_d2{f.Ls[o], f.Ls[o1]};
            rm = series_d2{q[om], q[om + (o1 - o)]};
            rp = series_d2{q[op], q[op + (o1 - o)]};
        }
        const double before = q[o - 1];
        CellIn c;
        RhoCross s;
        c.rho = in[0].x; c.jx = in[1].x; c.jy = in[2].x; c.h = in[3].x; c.hx = in[4].x; c.hy = in[5].x; c.Ls = in[6].x;
        s.xm = rm.x; s.xp = rp.x; s.ym = before; s.yp = in[0].y;
        cell(c, s, iy);
        if (two) {
            c.rho = in[0].y; c.jx = in[1].y; c.jy = in[2].y; c.h = in[3].y; c.hx = in[4].y; c.hy = in[5].y; c.Ls = in[6].y;
            s.xm = rm.y; s.xp = rp.y; s.ym = in[0].x; s.yp = q[o + 2];
            cell(c, s, iy + 1);
        }
    }
}

// A thread's (a row's, a record's) N sums
template <int N> struct RowAcc {
    double v[N];
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = 0.0;
    }
};

// Sum of the 256 threads' sets, valid in thread 0: lanes fold 32, 16, .. 1 apart, then waves 0, 1, 2, 3 in order
template <int N> __device__ __forceinline__ RowAcc<N> block_sum(RowAcc<N> a, double (*sm)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k)
        for (int s = 32; s >= 1; s >>= 1) a.v[k] += __shfl_down(a.v[k], s);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) sm[w][k] = a.v[k];
    }
    __syncthreads();
    RowAcc<N> r;
    r.zero();
    if (threadIdx.x == 0) {
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int k = 0; k < N; ++k) r.v[k] += sm[i][k];
        }
    }
    return r;
}

// A fold thread's sums of the rows' vectors part[k][nrow][N]: thread t adds rows t, t + 256, ... in order to +0.0; each_row(row)
// behind each, for what a series keeps beside the sums
template <int N, class Row> __device__ __forceinline__ RowAcc<N> add_rows(const double* part, int k, int nrow, Row each_row) {
    RowAcc<N> a;
    a.zero();
    for (int row = threadIdx.x; row < nrow; row += 256) {
        const double* in = part + ((long long)k * nrow + row) * N;
#pragma unroll
        for (int k = 0; k < N; ++k) a.v[k] += in[k];
        each_row(row);
    }
    return a;
}

// Sum of the rows' vectors, valid in thread 0: add_rows, then block_sum
template <int N> __device__ __forceinline__ RowAcc<N> fold_rows(const double* part, int k, int nrow, double (*sm)[N]) {
    return block_sum(add_rows<N>(part, k, nrow, [](int) {}), sm);
}

// Which step a one-workgroup kernel (small_kernel.hip, mid_kernel.hip) records next and where: the first multiple of the stride
// beyond the count the launch starts at, and its rank among the multiples in (base, .]; each record moves both on, without a
// division per step.  Only the stride is kept beside them: a record fetches its arguments when it is due, so that nothing of
// them stays in registers over the steps in between.
struct SeriesCursor {
    long long every, next, slot;
    __device__ __forceinline__ void begin(long long stride, long long step, long long base) {
        every = stride;
        next = (step / every + 1) * every;
        slot = next / every - base / every - 1;
    }
    __device__ __forceinline__ bool due(long long step) const { return step == next; }
    __device__ __forceinline__ void advance() { next += every; slot += 1; }
};

// cell index t -> (ix, iy) in rows of w cells for the cells one thread of nt visits: t = tid, tid + nt, ... without a division per
// cell (mid_kernel.hip walks its planes with it, extrema_kernels.hip: extrema_record_wide the interior)
struct MidCursor {
    int ix, iy, dq, dr, w;
    __device__ __forceinline__ MidCursor(int tid, int nt, int w_) : ix(tid / w_), iy(tid % w_), dq(nt / w_), dr(nt % w_), w(w_) {}
    __device__ __forceinline__ void next() {
        ix += dq; iy += dr;
        if (iy >= w) { iy -= w; ix += 1; }
    }
};

}  // namespace gpf
