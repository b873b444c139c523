// Reduced frames (frame_kernels.hip, api_frames.inc): which rule a window, a stride or a field mask breaks, how many output points
// a frame has, how the window is cut into blocks with their ragged ends, where a value sits in a record, which workgroup of the
// mean kernel takes which blocks, and how many steps a batch may hold while the record buffer is bounded.  Like lines.hpp this
// header compiles for the host on its own -- it includes lines.hpp alone, for the capacity arithmetic -- so that the device
// kernels, the library's argument checks and a stand-alone host program (tests/test_frames_hostcheck.py) evaluate the very same
// lines.
//
// A frame {mask, ix0, ix1, iy0, iy1, sx, sy, reduce, f4}: bit f of `mask` selects field f of the lines' nine (lines.hpp: rho jx jy
// p h tau_xz_bot tau_yz_bot tau_xz_top tau_yz_top); the window is inclusive in 1-based interior indices; the window is cut into
// blocks of sx x sy cells from its corner (ix0, iy0): block (a, b) holds the rows ix0 + a sx .. and the columns iy0 + b sy ..,
// clipped to the window, so the last block of an axis may be ragged.  mx = ceil((ix1 - ix0 + 1) / sx), my likewise.
//
// Record layout: [field in mask order][a][b], mx * my values per field, of float (f4) or double.
//
// reduce 0 (sample): the value of the block's first cell (ix0 + a sx, iy0 + b sy); no arithmetic, a -0.0 stays a -0.0.
// reduce 1 (mean), each field's term on its own:
//   1. per column c of the block, s_c starts at +0.0 and the block's rows are added in ascending ix;
//   2. S starts at +0.0 and the s_c are added in ascending iy;
//   3. the result is S / (double)(rows * cols), one division.
// mean with sx = sy = 1 is stored as sample (frame_normalise).  Who adds what depends on (window, stride) alone.
//
// The mean kernel's workgroups: group g of block-row a takes the frame_group_blocks(sy) = floor(256 / sy) whole blocks
// b = g * that .. along y, one lane per input column, so no block straddles two workgroups.
#pragma once

#include "lines.hpp"

namespace gpf {

constexpr int FRAME_NF = LINE_NF;
constexpr int FRAME_MAX_STRIDE = 64;
constexpr int FRAME_THREADS = 256;          // lanes of a workgroup of the mean kernel: input columns it takes at most
constexpr int FRAME_ALL = (1 << FRAME_NF) - 1;
constexpr int FRAME_TAU = 0x1e0;            // the four wall stresses: cell_fields is evaluated only if one is selected
constexpr int FRAME_GAP = 0x1f0;            // h and the stresses: the gap and the slip length are loaded only if one is selected
enum { FRAME_SAMPLE = 0, FRAME_MEAN = 1 };

// One frame as the device reads it
struct FrameSpec {
    int mask;                   // bit f: field f of the nine
    int ix0, ix1, iy0, iy1;     // the window, inclusive, 1-based interior indices
    int sx, sy;                 // the block
    int reduce;                 // FRAME_SAMPLE / FRAME_MEAN
    int f4;                     // 1: float records, 0: double
};

// What gpf_frames_set accepts: 0 if the frame is well formed on an Nx x Ny interior, else which rule it breaks -- 1 no field or a
// bit beyond the nine, 2 window outside the interior or reversed, 3 a stride outside 1..64, 4 `reduce` neither sample nor mean,
// 5 `f4` neither 0 nor 1
GPF_LINE_HD int frame_check(const FrameSpec& s, int Nx, int Ny) {
    if (s.mask < 1 || s.mask > FRAME_ALL) return 1;
    if (s.ix0 < 1 || s.ix1 > Nx || s.ix0 > s.ix1 || s.iy0 < 1 || s.iy1 > Ny || s.iy0 > s.iy1) return 2;
    if (s.sx < 1 || s.sx > FRAME_MAX_STRIDE || s.sy < 1 || s.sy > FRAME_MAX_STRIDE) return 3;
    if (s.reduce != FRAME_SAMPLE && s.reduce != FRAME_MEAN) return 4;
    if (s.f4 != 0 && s.f4 != 1) return 5;
    return 0;
}

// A mean over blocks of one cell is the cell: stored, and computed, as sample
GPF_LINE_HD void frame_normalise(FrameSpec& s) {
    if (s.reduce == FRAME_MEAN && s.sx == 1 && s.sy == 1) s.reduce = FRAME_SAMPLE;
}

GPF_LINE_HD int frame_mx(const FrameSpec& s) { return (s.ix1 - s.ix0 + s.sx) / s.sx; }
GPF_LINE_HD int frame_my(const FrameSpec& s) { return (s.iy1 - s.iy0 + s.sy) / s.sy; }

// First row / column of block a / b, and how many of them lie in the window (the last block's may be fewer than the stride)
GPF_LINE_HD int frame_row0(const FrameSpec& s, int a) { return s.ix0 + a * s.sx; }
GPF_LINE_HD int frame_col0(const FrameSpec& s, int b) { return s.iy0 + b * s.sy; }
GPF_LINE_HD int frame_block_rows(const FrameSpec& s, int a) { const int left = s.ix1 - frame_row0(s, a) + 1; return left < s.sx ? left : s.sx; }
GPF_LINE_HD int frame_block_cols(const FrameSpec& s, int b) { const int left = s.iy1 - frame_col0(s, b) + 1; return left < s.sy ? left : s.sy; }

GPF_LINE_HD int frame_fields(int mask) {
    int n = 0;
    for (int f = 0; f < FRAME_NF; ++f) n += (mask >> f) & 1;
    return n;
}
// Rank of the selected field f among the selected ones: its place in the record
GPF_LINE_HD int frame_rank(int mask, int f) { return frame_fields(mask & ((1 << f) - 1)); }

// Index of (field of rank r, block a, block b) inside a record, in values
GPF_LINE_HD long long frame_at(int r, int a, int b, int mx, int my) { return ((long long)r * mx + a) * my + b; }
GPF_LINE_HD long long frame_values(const FrameSpec& s) { return (long long)frame_fields(s.mask) * frame_mx(s) * frame_my(s); }
GPF_LINE_HD long long frame_record_bytes(const FrameSpec& s) { return frame_values(s) * (s.f4 ? 4 : 8); }

// The mean kernel: whole blocks a workgroup takes along y, the workgroups of a block-row, the first block of group g and the input
// columns it reads (clipped to the window)
GPF_LINE_HD int frame_group_blocks(int sy) { return FRAME_THREADS / sy; }
GPF_LINE_HD int frame_groups(const FrameSpec& s) { const int nb = frame_group_blocks(s.sy); return (frame_my(s) + nb - 1) / nb; }
GPF_LINE_HD int frame_group_block0(const FrameSpec& s, int g) { return g * frame_group_blocks(s.sy); }
GPF_LINE_HD int frame_group_cols(const FrameSpec& s, int g) {
    const int first = frame_col0(s, frame_group_block0(s, g)), most = frame_group_blocks(s.sy) * s.sy, left = s.iy1 - first + 1;
    return left < most ? left : most;
}
// Where column t of a group's run keeps its sum in LDS: one double of padding per 32, so that the threads that add a block's
// columns (sy doubles apart) do not meet in one bank
GPF_LINE_HD int frame_lds_at(int t) { return t + (t >> 5); }
constexpr int FRAME_LDS_COLS = FRAME_THREADS + FRAME_THREADS / 32;

// Records the device buffer holds by default, and the steps a batch may hold: the lines' arithmetic on a record's bytes
GPF_LINE_HD long long frames_default_capacity(long long budget_bytes, long long record_bytes, long long log_cap, long long every) {
    return lines_default_capacity(budget_bytes, (record_bytes + 7) / 8, log_cap, every);
}
GPF_LINE_HD long long frames_batch_limit(long long base, long long every, long long capacity) { return lines_batch_limit(base, every, capacity); }

}  // namespace gpf
