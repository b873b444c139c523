// Reduced frames of the committed state (entry points in api_frames.inc): for each selected field of the lines' nine -- rho, jx, jy,
// p, h and the four wall shear stresses, line_kernels.hip: line_terms' definitions and its __builtin_canonicalize -- one (mx, my)
// array over a window of the interior, sampled at the first cell of every sx x sy block or averaged over the block, stored as
// double or float: the picture of the film at a recorded step, without a plane leaving the device.
//
// frame_terms<EOS, NEED_TAU> evaluates a cell's terms: rho, jx, jy and p always (24 B per cell), h from plane 0 of the gap if it is
// selected, and with NEED_TAU -- a wall stress is selected -- the three gap planes, the slip length and cell_fields<EOS>.  Terms that
// are not selected are never added nor stored; the mask is uniform, so the branches on it are scalar.
//
// Launches per record, both guarded by the device's run state (series_rows.hpp: series_skip) like k_line_point:
//   k_frame_sample   one thread per output point (a = blockIdx.y, lanes contiguous in b): the block's first cell, no arithmetic.
//   k_frame_mean     one workgroup per (block-row a = blockIdx.y, group of floor(256 / sy) whole blocks along y): lane t owns the
//                    input column frame_col0(first block) + t, so the loads of a row are contiguous 8-byte loads; it adds the
//                    block's rows in ascending ix to +0.0 with the selected fields' sums in registers and puts them in LDS as
//                    [field][column]; behind a barrier thread j adds the sy column sums of block j in ascending iy to +0.0, divides
//                    once by (double)(rows * cols), converts and stores.  18.6 KB of LDS per workgroup, eight workgroups per CU.
// The order is stated in frames.hpp.  No atomics, no arrival order: a record is a pure function of the state and the frame.
#pragma once

#include "frames.hpp"
#include "series_rows.hpp"

namespace gpf {

struct FrameArgs {
    const double *qa, *qb, *topo, *Ls;
    const StepState* st;
    char* rec;              // [cap + 1][record_bytes]
    Layout L;
    FrameSpec s;
    int mx, my;
    long long record_bytes;
    long long slot, cap;    // record to write; slots the buffer holds besides the one of gpf_frames_now
};

// One cell's terms in the record's order; those a frame cannot select with this instantiation, or does not, are +0.0
template <int EOS, bool HAS_LS, bool NEED_TAU>
__device__ __forceinline__ LineVals frame_terms(const FrameArgs& f, const double* q, const Phys& P, int ix, int iy) {
    const long long o = f.L.at(ix, iy);
    LineVals t;
    CellIn c;
    c.rho = q[o]; c.jx = q[f.L.plane + o]; c.jy = q[2 * f.L.plane + o];
    t.v[0] = c.rho; t.v[1] = c.jx; t.v[2] = c.jy;
    t.v[3] = __builtin_canonicalize(eos_pressure<EOS>(c.rho, P));
#pragma unroll
    for (int n = 4; n < FRAME_NF; ++n) t.v[n] = 0.0;
    if (NEED_TAU) {
        c.h = f.topo[o]; c.hx = f.topo[f.L.plane + o]; c.hy = f.topo[2 * f.L.plane + o];
        c.Ls = HAS_LS ? f.Ls[o] : 0.0;
        CellFields w;
        cell_fields<EOS>(c, P, w);
        t.v[4] = c.h;
        t.v[5] = __builtin_canonicalize(w.lower[4]); t.v[6] = __builtin_canonicalize(w.lower[3]);
        t.v[7] = __builtin_canonicalize(w.upper[4]); t.v[8] = __builtin_canonicalize(w.upper[3]);
    } else if (f.s.mask & (1 << 4)) {
        t.v[4] = f.topo[o];
    }
    return t;
}

// The selected value of rank r at (a, b), as the record's dtype
__device__ __forceinline__ void frame_store(const FrameArgs& f, int r, int a, int b, double v) {
    char* out = f.rec + f.slot * f.record_bytes;
    const long long at = frame_at(r, a, b, f.mx, f.my);
    if (f.s.f4) reinterpret_cast<float*>(out)[at] = (float)v;       // one conversion, round to nearest even
    else reinterpret_cast<double*>(out)[at] = v;
}

template <int EOS, bool HAS_LS, bool NEED_TAU>
__global__ __launch_bounds__(FRAME_THREADS) void k_frame_sample(const FrameArgs f, const Phys P, long long expect) {
    if (series_skip(f.st, expect, f.slot, f.cap)) return;
    const int a = blockIdx.y, b = blockIdx.x * FRAME_THREADS + threadIdx.x;
    if (a >= f.mx || b >= f.my) return;
    const double* q = f.st->parity ? f.qb : f.qa;
    const LineVals t = frame_terms<EOS, HAS_LS, NEED_TAU>(f, q, P, frame_row0(f.s, a), frame_col0(f.s, b));
    int r = 0;
#pragma unroll
    for (int n = 0; n < FRAME_NF; ++n) {
        if (!(f.s.mask & (1 << n))) continue;
        frame_store(f, r, a, b, t.v[n]);
        ++r;
    }
}

template <int EOS, bool HAS_LS, bool NEED_TAU>
__global__ __launch_bounds__(FRAME_THREADS) void k_frame_mean(const FrameArgs f, const Phys P, long long expect) {
    __shared__ double sums[FRAME_NF][FRAME_LDS_COLS];
    if (series_skip(f.st, expect, f.slot, f.cap)) return;
    const int a = blockIdx.y, g = blockIdx.x, t = threadIdx.x;
    if (a >= f.mx || g >= frame_groups(f.s)) return;                // the whole workgroup
    const int b0 = frame_group_block0(f.s, g), ncol = frame_group_cols(f.s, g);
    const int rows = frame_block_rows(f.s, a);
    if (t < ncol) {
        const double* q = f.st->parity ? f.qb : f.qa;
        const int ix = frame_row0(f.s, a), iy = frame_col0(f.s, b0) + t;
        LineVals s;
#pragma unroll
        for (int n = 0; n < FRAME_NF; ++n) s.v[n] = 0.0;
        for (int r = 0; r < rows; ++r) {
            const LineVals v = frame_terms<EOS, HAS_LS, NEED_TAU>(f, q, P, ix + r, iy);
#pragma unroll
            for (int n = 0; n < FRAME_NF; ++n)
                if ((NEED_TAU || n <= 4) && (f.s.mask & (1 << n))) s.v[n] += v.v[n];
        }
#pragma unroll
        for (int n = 0; n < FRAME_NF; ++n)
            if ((NEED_TAU || n <= 4) && (f.s.mask & (1 << n))) sums[n][frame_lds_at(t)] = s.v[n];
    }
    __syncthreads();
    const int b = b0 + t;
    if (t >= frame_group_blocks(f.s.sy) || b >= f.my) return;
    const int cols = frame_block_cols(f.s, b), first = t * f.s.sy;
    const double cells = (double)(rows * cols);
    int r = 0;
#pragma unroll
    for (int n = 0; n < FRAME_NF; ++n) {
        if (!(f.s.mask & (1 << n))) continue;
        double S = 0.0;
        if (NEED_TAU || n <= 4)
            for (int c = 0; c < cols; ++c) S += sums[n][frame_lds_at(first + c)];
        frame_store(f, r, a, b, S / cells);
        ++r;
    }
}

}  // namespace gpf
