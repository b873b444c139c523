// Line profiles of the committed state (entry points in api_lines.inc): for each of K <= 8 lines the nine fields rho, jx, jy, p, h
// and the four wall shear stresses along the interior rows (a line along x) or columns (along y), at one column / row or as the
// arithmetic mean over a band of them -- what the reference's viz/plotting.py: plot_frame(dim=1) and viz/animations.py draw of a
// 2-D run, recorded behind the committed steps without a frame leaving the device.
//
// p is closures.hpp: eos_pressure<EOS> of the committed density -- the function k_probe_record calls, so a probe on the line's
// cell holds the same bits --, h plane 0 of the gap, the stresses lower[4], lower[3], upper[4], upper[3] of cell_fields<EOS>: the
// terms integral_kernels.hip: film_cell adds.  line_terms evaluates the nine for one cell and hands each through
// __builtin_canonicalize, the identity on the values, which keeps the backend (the library is compiled with -ffp-contract=fast)
// from fusing a term's last multiplication into a band's addition: a band therefore adds exactly the bits a single-index line
// stores (weighted_kernels.hip has the same construction and the ISA evidence).
//
// Launches per record, all guarded by the device's run state like k_film_partial, grid.y = the line, a workgroup whose line is of
// another kind returns at once (the host launches a kind only if a line of it is armed):
//   k_line_point          single-index lines: one thread per point.  Along y the loads are contiguous; along x each lane touches
//                         its own cache line (stride pitch), Nx lines per plane.
//   k_line_band_x         bands along x: one wave per interior row (four per workgroup); lane l adds the cells i0 + l, i0 + l + 64,
//                         ... ascending, the lanes fold 32 .. 1 apart with __shfl_down, lane 0 divides by (double)n and stores.
//   k_line_band_y_partial bands along y: one thread per (chunk of 32 rows, iy), lanes contiguous in iy; the chunk's rows are added
//                         ascending and the nine sums stored to scratch[chunk][field][iy].
//   k_line_band_y_fold    one thread per iy adds the chunk sums ascending, divides by (double)n and stores.
// The order is stated in lines.hpp.  No atomics, no arrival order, no LDS: a record is a pure function of the state and the lines.
#pragma once

#include "lines.hpp"

namespace gpf {

struct LineArgs {
    const double *qa, *qb, *topo, *Ls;
    const StepState* st;
    double* rec;            // [cap + 1][rec_doubles]
    double* scratch;        // chunk sums of the bands along y
    Layout L;
    int K;
    long long rec_doubles;
    long long slot, cap;    // record to write; slots the buffer holds besides the one of gpf_lines_now
    Line lines[LINE_MAX_K];
};

template <bool HAS_LS>
__device__ __forceinline__ CellIn line_load(const LineArgs& f, const double* q, int ix, int iy) {
    const long long o = f.L.at(ix, iy);
    CellIn c;
    c.rho = q[o]; c.jx = q[f.L.plane + o]; c.jy = q[2 * f.L.plane + o];
    c.h = f.topo[o]; c.hx = f.topo[f.L.plane + o]; c.hy = f.topo[2 * f.L.plane + o];
    c.Ls = HAS_LS ? f.Ls[o] : 0.0;
    return c;
}

struct LineVals {
    double v[LINE_NF];
};

// One cell's nine values, in the record's order
template <int EOS>
__device__ __forceinline__ LineVals line_terms(const CellIn& c, const Phys& P) {
    CellFields o;
    cell_fields<EOS>(c, P, o);
    LineVals t;
    t.v[0] = c.rho; t.v[1] = c.jx; t.v[2] = c.jy;
    t.v[3] = __builtin_canonicalize(eos_pressure<EOS>(c.rho, P));
    t.v[4] = c.h;
    t.v[5] = __builtin_canonicalize(o.lower[4]); t.v[6] = __builtin_canonicalize(o.lower[3]);
    t.v[7] = __builtin_canonicalize(o.upper[4]); t.v[8] = __builtin_canonicalize(o.upper[3]);
    return t;
}

// Uniform guards of every kernel: the step did not run or was rolled back; a slot outside the buffer; a line that is not there
__device__ __forceinline__ bool line_skip(const LineArgs& f, long long expect, int k) {
    if (f.st->step != expect || f.st->invalid != 0) return true;
    if (f.slot < 0 || f.slot > f.cap) return true;
    return k >= f.K;
}

template <int EOS, bool HAS_LS>
__global__ __launch_bounds__(256) void k_line_point(const LineArgs f, const Phys P, long long expect) {
    const int k = blockIdx.y;
    if (line_skip(f, expect, k)) return;
    const Line l = f.lines[k];
    if (line_is_band(l)) return;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= l.len) return;
    const double* q = f.st->parity ? f.qb : f.qa;
    const int ix = l.along == 0 ? 1 + j : l.i0, iy = l.along == 0 ? l.i0 : 1 + j;
    const LineVals t = line_terms<EOS>(line_load<HAS_LS>(f, q, ix, iy), P);
    double* out = f.rec + f.slot * f.rec_doubles;
#pragma unroll
    for (int n = 0; n < LINE_NF; ++n) out[line_at(l, n, j)] = t.v[n];
}

template <int EOS, bool HAS_LS>
__global__ __launch_bounds__(256) void k_line_band_x(const LineArgs f, const Phys P, long long expect) {
    const int k = blockIdx.y;
    if (line_skip(f, expect, k)) return;
    const Line l = f.lines[k];
    if (l.along != 0 || !line_is_band(l)) return;
    const int lane = threadIdx.x & (LINE_LANES - 1), j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= l.len) return;                     // the whole wave
    const double* q = f.st->parity ? f.qb : f.qa;
    LineVals a;
#pragma unroll
    for (int n = 0; n < LINE_NF; ++n) a.v[n] = 0.0;
    for (int iy = l.i0 + lane; iy <= l.i1; iy += LINE_LANES) {
        const LineVals t = line_terms<EOS>(line_load<HAS_LS>(f, q, 1 + j, iy), P);
#pragma unroll
        for (int n = 0; n < LINE_NF; ++n) a.v[n] += t.v[n];
    }
#pragma unroll
    for (int n = 0; n < LINE_NF; ++n)
        for (int s = 32; s >= 1; s >>= 1) a.v[n] += __shfl_down(a.v[n], s);
    if (lane != 0) return;
    const double cells = (double)line_band_cells(l);
    double* out = f.rec + f.slot * f.rec_doubles;
#pragma unroll
    for (int n = 0; n < LINE_NF; ++n) out[line_at(l, n, j)] = a.v[n] / cells;
}

template <int EOS, bool HAS_LS>
__global__ __launch_bounds__(256) void k_line_band_y_partial(const LineArgs f, const Phys P, long long expect) {
    const int k = blockIdx.y;
    if (line_skip(f, expect, k)) return;
    const Line l = f.lines[k];
    if (l.along != 1 || !line_is_band(l)) return;
    const int cells = line_band_cells(l);
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)line_chunks(cells) * l.len) return;
    const int c = (int)(t / l.len), j = (int)(t - (long long)c * l.len);
    const double* q = f.st->parity ? f.qb : f.qa;
    LineVals a;
#pragma unroll
    for (int n = 0; n < LINE_NF; ++n) a.v[n] = 0.0;
    const int first = l.i0 + c * LINE_CHUNK, rows = line_chunk_rows(cells, c);
    for (int r = 0; r < rows; ++r) {
        const LineVals v = line_terms<EOS>(line_load<HAS_LS>(f, q, first + r, 1 + j), P);
#pragma unroll
        for (int n = 0; n < LINE_NF; ++n) a.v[n] += v.v[n];
    }
    double* out = f.scratch + l.scratch_off + (long long)c * LINE_NF * l.len + j;
#pragma unroll
    for (int n = 0; n < LINE_NF; ++n) out[(long long)n * l.len] = a.v[n];
}

__global__ __launch_bounds__(256) void k_line_band_y_fold(const LineArgs f, long long expect) {
    const int k = blockIdx.y;
    if (line_skip(f, expect, k)) return;
    const Line l = f.lines[k];
    if (l.along != 1 || !line_is_band(l)) return;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= l.len) return;
    const int cells = line_band_cells(l), nch = line_chunks(cells);
    LineVals a;
#pragma unroll
    for (int n = 0; n < LINE_NF; ++n) a.v[n] = 0.0;
    for (int c = 0; c < nch; ++c) {
        const double* in = f.scratch + l.scratch_off + (long long)c * LINE_NF * l.len + j;
#pragma unroll
        for (int n = 0; n < LINE_NF; ++n) a.v[n] += in[(long long)n * l.len];
    }
    double* out = f.rec + f.slot * f.rec_doubles;
#pragma unroll
    for (int n = 0; n < LINE_NF; ++n) out[line_at(l, n, j)] = a.v[n] / (double)cells;
}

}  // namespace gpf
