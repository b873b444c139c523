// Line profiles (line_kernels.hip, api_lines.inc): where a line's values sit in a record, how a band is cut into the pieces that
// are added, and how many steps a batch may hold while the record buffer is bounded.  This header compiles for the host on its own
// -- it includes nothing of the project -- so that the device kernels, the library's argument checks and a stand-alone host
// program (tests/test_lines_hostcheck.py) evaluate the very same lines.
//
// A line {along, i0, i1} in 1-based interior indices:
//   along 0 (x)  a profile over the interior rows ix = 1..Nx (length Nx), taken at column i0 = i1, or the arithmetic mean over
//                the columns i0..i1 inclusive;
//   along 1 (y)  a profile over the interior columns iy = 1..Ny (length Ny), at row i0 = i1 or averaged over the rows i0..i1.
// i0 == i1 is a single-index line: the nine values of the cell itself, no addition and no division (a -0.0 stays a -0.0).
//
// Record layout: for each line in order, LINE_NF = 9 fields (rho jx jy p h tau_xz_bot tau_yz_bot tau_xz_top tau_yz_top), each
// `length` doubles: value (line k, field f, point j) at line_offset(k) + f * length_k + j, j = 0 .. length_k - 1.
//
// Order of a band's additions (n = i1 - i0 + 1 cells per point; every sum starts from +0.0 and each of the nine terms is added
// on its own):
//   along x   per row ix one wave: lane l = 0..63 adds the cells iy = i0 + l, i0 + l + 64, ... <= i1 in ascending order; the 64
//             lane sums are folded 32, 16, 8, 4, 2, 1 apart (lane l += lane l + s for l < s); lane 0 divides by (double)n.
//   along y   per column iy: chunk c = 0 .. line_chunks(n) - 1 holds the LINE_CHUNK = 32 consecutive rows from i0 + 32 c (the
//             last chunk the rest); a chunk's rows are added in ascending order, then the chunk sums in ascending order, then
//             the total is divided by (double)n.
// Who adds what, and in which order, depends on (Nx, Ny, line) alone.
#pragma once

#if defined(__HIPCC__)
#define GPF_LINE_HD __host__ __device__ __forceinline__
#else
#define GPF_LINE_HD inline
#endif

namespace gpf {

constexpr int LINE_MAX_K = 8;
constexpr int LINE_NF = 9;              // rho jx jy p h tau_xz_bot tau_yz_bot tau_xz_top tau_yz_top
constexpr int LINE_CHUNK = 32;          // rows per partial sum of a band along y
constexpr int LINE_LANES = 64;          // lanes that share a row of a band along x

// One line as the device reads it
struct Line {
    int along;                  // 0: x, 1: y
    int i0, i1;                 // the column(s) of a line along x, the row(s) of one along y
    int len;                    // Nx along x, Ny along y
    long long rec_off;          // line_offset: doubles before this line in a record
    long long scratch_off;      // doubles before this line's chunk sums in the scratch buffer (bands along y)
};

GPF_LINE_HD int line_length(int along, int Nx, int Ny) { return along == 0 ? Nx : Ny; }

// The reference's centre line: column ny // 2 of the ghosted frame with ny = Ny + 2 (row nx // 2 along y)
GPF_LINE_HD int line_centre(int along, int Nx, int Ny) { return along == 0 ? (Ny + 2) / 2 : (Nx + 2) / 2; }

// What gpf_lines_set accepts: 0 if the line is well formed on an Nx x Ny interior, else which rule it breaks --
// 1 `along` is neither 0 nor 1, 2 indices outside the interior or reversed
GPF_LINE_HD int line_check(int along, int i0, int i1, int Nx, int Ny) {
    if (along != 0 && along != 1) return 1;
    const int n = along == 0 ? Ny : Nx;             // the axis the indices count along
    if (i0 < 1 || i1 > n || i0 > i1) return 2;
    return 0;
}

GPF_LINE_HD bool line_is_band(const Line& l) { return l.i1 > l.i0; }
GPF_LINE_HD int line_band_cells(const Line& l) { return l.i1 - l.i0 + 1; }
GPF_LINE_HD int line_chunks(int n) { return (n + LINE_CHUNK - 1) / LINE_CHUNK; }
// rows of chunk c of a band of n rows
GPF_LINE_HD int line_chunk_rows(int n, int c) { const int left = n - c * LINE_CHUNK; return left < LINE_CHUNK ? left : LINE_CHUNK; }

GPF_LINE_HD long long line_doubles(int len) { return (long long)LINE_NF * len; }
// doubles the chunk sums of a band along y take: [chunk][field][Ny]
GPF_LINE_HD long long line_scratch_doubles(const Line& l) {
    return (l.along == 1 && line_is_band(l)) ? (long long)line_chunks(line_band_cells(l)) * LINE_NF * l.len : 0;
}

// Fills len, rec_off and scratch_off of the K lines; returns the doubles of one record, *scratch the doubles of the scratch buffer
GPF_LINE_HD long long lines_layout(Line* lines, int K, int Nx, int Ny, long long* scratch) {
    long long rec = 0, scr = 0;
    for (int k = 0; k < K; ++k) {
        lines[k].len = line_length(lines[k].along, Nx, Ny);
        lines[k].rec_off = rec;
        lines[k].scratch_off = scr;
        rec += line_doubles(lines[k].len);
        scr += line_scratch_doubles(lines[k]);
    }
    if (scratch) *scratch = scr;
    return rec;
}

// Index of (field f, point j) of a line inside a record
GPF_LINE_HD long long line_at(const Line& l, int f, int j) { return l.rec_off + (long long)f * l.len + j; }

// Records a stepping call leaves for the steps (base, base + ran]: the multiples of `every` among them
GPF_LINE_HD long long lines_count(long long base, long long ran, long long every) {
    return ran > 0 ? (base + ran) / every - base / every : 0;
}

// Default number of records the device buffer holds: as many as fit `budget_bytes`, at least 1, at most what the longest batch
// (log_cap steps) can leave at this stride
GPF_LINE_HD long long lines_default_capacity(long long budget_bytes, long long record_doubles, long long log_cap, long long every) {
    long long c = budget_bytes / (record_doubles * 8);
    const long long most = (log_cap + every - 1) / every;
    if (c > most) c = most;
    if (c < 1) c = 1;
    return c;
}

// Steps a batch that begins at step count `base` may hold so that it leaves at most `capacity` records: capacity * every less the
// steps since the last recorded one.  Always >= 1, and the batch that takes them all ends on a recorded step or earlier.
GPF_LINE_HD long long lines_batch_limit(long long base, long long every, long long capacity) {
    return capacity * every - base % every;
}

}  // namespace gpf
