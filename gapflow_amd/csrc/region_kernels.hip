// Region series of the committed state (entry points in api_regions.inc): for each of K <= 8 regions {field, lo, hi, box} the
// weighted film integrals' nine sums (weighted_kernels.hip: p h rho_h jx_h jy_h and the four wall shear stresses) over the
// interior cells whose `field` lies in [lo, hi) and which lie in `box`, the exact number of those cells and their bounding box.
// A region is a zone the state of the step defines -- the cavitated zone rho < rho_cav, the thin film h < c, the area above a
// pressure limit -- so no plane fixed in advance can stand for it: the 0 / 1 weight is evaluated per cell from the state
// (regions.hpp, which also compiles for the host), and nothing is uploaded or stored per cell.
//
// The two launches per record, the pair walk, the fold tree and the guard are series_rows.hpp's, as for the weighted integrals:
//   k_region_partial   grid (Nx, K): one workgroup per interior row ix and region k; each cell goes through wfilm_cell with the
//                      weight 1.0 (member) or 0.0 (not).  Beside the sums every thread counts its members and keeps the least and
//                      the largest iy among them; shuffles and the four waves' slots fold these integers.  Thread 0 stores the row's
//                      nine doubles to part[k][ix - 1][9] and (count, iy_min, iy_max) to ipart[k][ix - 1][3], with plain stores.
//   k_region_fold      grid (K): the rows' doubles through add_rows, in the same loop the counts added, iy_min / iy_max by min / max, ix_min /
//                      ix_max from the rows whose count is not zero; thread 0 applies dx dy and stores the slot: nine doubles to
//                      rec[slot][k][9] and (cells, ix_min, ix_max, iy_min, iy_max) as int64 to irec[slot][k][5], all -1 behind
//                      cells = 0.
// The doubles go through weighted_kernels.hip's own functions in its own order with a weight of exactly 1.0 or 0.0, so on a
// finite state the nine sums equal, in every bit, what k_wfilm_partial / k_wfilm_fold give for the 0 / 1 plane of the same
// predicate: acc += canonicalize(w * term) adds the term's own bits, or a zero.  (On a state that is not finite a
// cell outside the region still enters as 0 * term, a NaN for a term that is NaN or infinite, exactly as behind a weight plane.)
// The count and the bounding box are integer folds: their order is free and their result exact.  No floating-point atomics, no
// arrival order, no ticket: a record is a pure function of the state and the region list.
// `p` in a predicate is eos_pressure<EOS> of the committed density -- the p of the probes, the extrema and the statistics, not
// film_pressure, which the first of the nine sums adds --, `h` plane 0 of the gap, rho / jx / jy the planes of q[parity].  It is
// evaluated only by the workgroups of a region that asks for it.  One plane fewer than k_wfilm_partial reads: there is no weight
// plane.
#pragma once

#include "regions.hpp"
#include "series_rows.hpp"

namespace gpf {

constexpr int REGION_NROW = 3;          // a row's integers: count iy_min iy_max
constexpr int REGION_NONE_MIN = 0x7fffffff, REGION_NONE_MAX = -1;      // iy_min / iy_max (ix_min / ix_max) of no cell

struct RegionArgs {
    const double *qa, *qb, *topo, *Ls;
    const Region* regions;  // [K], device memory
    const StepState* st;
    double* part;           // [K][Nx][WFILM_NQ]
    int* ipart;             // [K][Nx][REGION_NROW]
    double* rec;            // [cap + 1][K][WFILM_NQ]
    long long* irec;        // [cap + 1][K][REGION_NI]
    Layout L;
    double dx, dy;
    int K;
    int wide;               // 16-byte pair loads are aligned
    long long slot, cap;    // record to write; slots the buffers hold
};

// A thread's (a row's, a region's) integers
struct RegionInts {
    long long cells;
    int ix_min, ix_max, iy_min, iy_max;
    __device__ __forceinline__ void zero() {
        cells = 0; ix_min = iy_min = REGION_NONE_MIN; ix_max = iy_max = REGION_NONE_MAX;
    }
    __device__ __forceinline__ void merge(const RegionInts& o) {
        cells += o.cells;
        ix_min = min(ix_min, o.ix_min); ix_max = max(ix_max, o.ix_max);
        iy_min = min(iy_min, o.iy_min); iy_max = max(iy_max, o.iy_max);
    }
};

// The 256 threads' integers folded into wave slots sm[4]: call it BEFORE block_sum, whose barrier publishes the slots;
// region_ints_total then reads them (thread 0 needs the result).
__device__ __forceinline__ void region_ints_to_slots(RegionInts a, RegionInts* sm) {
    for (int s = 32; s >= 1; s >>= 1) {
        RegionInts o;
        o.cells = __shfl_down(a.cells, s);
        o.ix_min = __shfl_down(a.ix_min, s); o.ix_max = __shfl_down(a.ix_max, s);
        o.iy_min = __shfl_down(a.iy_min, s); o.iy_max = __shfl_down(a.iy_max, s);
        a.merge(o);
    }
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = a;
}

__device__ __forceinline__ RegionInts region_ints_total(const RegionInts* sm) {
    RegionInts r = sm[0];
    for (int i = 1; i < 4; ++i) r.merge(sm[i]);
    return r;
}

// The value a region's predicate tests in one cell
template <int EOS>
__device__ __forceinline__ double region_field(int field, const CellIn& c, const Phys& P) {
    switch (field) {
        case 0: return eos_pressure<EOS>(c.rho, P);
        case 1: return c.rho;
        case 2: return c.h;
        case 3: return c.jx;
        default: return c.jy;
    }
}

template <int EOS>
__device__ __forceinline__ void region_cell(WFilmAcc& a, RegionInts& n, const Region& r, const Phys& P, const CellIn& c, int ix, int iy) {
    const bool in = region_member(r, region_field<EOS>(r.field, c, P), ix, iy);
    wfilm_cell<EOS>(a, P, c, in ? 1.0 : 0.0);
    if (in) {
        n.cells += 1;
        n.iy_min = min(n.iy_min, iy); n.iy_max = max(n.iy_max, iy);
    }
}

template <int EOS, bool HAS_LS>
__global__ __launch_bounds__(256) void k_region_partial(const RegionArgs f, const Phys P, long long expect) {
    __shared__ double sm[4][WFILM_NQ];
    __shared__ RegionInts smi[4];
    if (series_skip(f.st, expect, f.slot, f.cap)) return;
    const Layout& L = f.L;
    const int ix = 1 + blockIdx.x, kr = blockIdx.y;
    if (ix > L.Nx || kr >= f.K) return;
    const Region r = f.regions[kr];
    WFilmAcc a;
    a.zero();
    RegionInts n;
    n.zero();
    row_pairs<FilmPlanes<HAS_LS>>(f, nullptr, ix, [&](const CellIn& c, double, int iy, double) { region_cell<EOS>(a, n, r, P, c, ix, iy); });
    region_ints_to_slots(n, smi);
    const WFilmAcc s = block_sum(a, sm);
    if (threadIdx.x == 0) {
        const long long row = (long long)kr * L.Nx + (ix - 1);
        double* out = f.part + row * WFILM_NQ;
#pragma unroll
        for (int k = 0; k < WFILM_NQ; ++k) out[k] = s.v[k];
        const RegionInts t = region_ints_total(smi);
        int* iout = f.ipart + row * REGION_NROW;
        iout[0] = (int)t.cells; iout[1] = t.iy_min; iout[2] = t.iy_max;
    }
}

__global__ __launch_bounds__(256) void k_region_fold(const RegionArgs f, long long expect) {
    __shared__ double sm[4][WFILM_NQ];
    __shared__ RegionInts smi[4];
    if (series_skip(f.st, expect, f.slot, f.cap)) return;
    const int kr = blockIdx.x;
    if (kr >= f.K) return;
    RegionInts n;
    n.zero();
    const WFilmAcc a = add_rows<WFILM_NQ>(f.part, kr, f.L.Nx, [&](int row) {
        const int* iin = f.ipart + ((long long)kr * f.L.Nx + row) * REGION_NROW;
        if (iin[0] > 0) {
            RegionInts o;
            o.cells = iin[0]; o.ix_min = o.ix_max = row + 1; o.iy_min = iin[1]; o.iy_max = iin[2];
            n.merge(o);
        }
    });
    region_ints_to_slots(n, smi);
    const WFilmAcc s = block_sum(a, sm);
    if (threadIdx.x != 0) return;
    double* out = f.rec + (f.slot * f.K + kr) * WFILM_NQ;
    const double dA = f.dx * f.dy;
#pragma unroll
    for (int k = 0; k < WFILM_NQ; ++k) out[k] = s.v[k] * dA;
    const RegionInts t = region_ints_total(smi);
    long long* iout = f.irec + (f.slot * f.K + kr) * REGION_NI;
    const bool none = t.cells == 0;
    iout[0] = t.cells;
    iout[1] = none ? -1 : t.ix_min; iout[2] = none ? -1 : t.ix_max;
    iout[3] = none ? -1 : t.iy_min; iout[4] = none ? -1 : t.iy_max;
}

}  // namespace gpf
