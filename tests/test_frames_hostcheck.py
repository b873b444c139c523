"""Reduced frames: the index and block arithmetic of gapflow_amd/csrc/frames.hpp -- the header the device kernels and the library's
argument checks include -- compiled for the host with a small program of its own (its own main) under AddressSanitizer and
UndefinedBehaviorSanitizer, and run directly.  Over a sweep of (Nx, Ny, window, stride), windows wider than one workgroup's run
at sy = 3 included, the program walks the mean kernel's workgroups, lanes and output threads as k_frame_mean does and the sample
kernel's threads as k_frame_sample does: every output index is written exactly once, every window cell is read by exactly one
lane and belongs to exactly one block, the block counts sum to the window, the LDS slots stay inside the array and apart; then
the argument check, the record's size, and the capacity / batch-limit arithmetic of gpf_step replayed over whole runs.  Nothing of
it is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <algorithm>
#include <cstdio>
#include <vector>
#include "frames.hpp"

static int failed = 0;
#define CHECK(expr) do { if (!(expr)) { std::printf("FAILED line %d: %s\n", __LINE__, #expr); ++failed; } } while (0)

using namespace gpf;

// One frame, walked as the kernels walk it: `cells` counts the reads of every window cell (indexed over the whole interior, so a
// read outside the window shows), `hits` the stores to every index of a record (the vectors are what the sanitizer watches)
static void walk(int Nx, int Ny, FrameSpec s) {
    CHECK(frame_check(s, Nx, Ny) == 0);
    const int mx = frame_mx(s), my = frame_my(s), nf = frame_fields(s.mask);
    CHECK(mx == (s.ix1 - s.ix0 + 1 + s.sx - 1) / s.sx && my == (s.iy1 - s.iy0 + 1 + s.sy - 1) / s.sy);
    CHECK(frame_values(s) == (long long)nf * mx * my && frame_record_bytes(s) == frame_values(s) * (s.f4 ? 4 : 8));
    std::vector<int> cells((size_t)Nx * Ny, 0), hits((size_t)frame_values(s), 0), block_of((size_t)Nx * Ny, -1);
    // the blocks: inside the window, their extents at least 1 and at most the stride, their cells sum to the window
    long long sum = 0;
    for (int a = 0; a < mx; ++a)
        for (int b = 0; b < my; ++b) {
            const int rows = frame_block_rows(s, a), cols = frame_block_cols(s, b);
            CHECK(rows >= 1 && rows <= s.sx && cols >= 1 && cols <= s.sy);
            CHECK((rows == s.sx) || a == mx - 1);
            CHECK((cols == s.sy) || b == my - 1);
            sum += (long long)rows * cols;
            for (int r = 0; r < rows; ++r)
                for (int c = 0; c < cols; ++c) {
                    const int ix = frame_row0(s, a) + r, iy = frame_col0(s, b) + c;
                    CHECK(ix >= s.ix0 && ix <= s.ix1 && iy >= s.iy0 && iy <= s.iy1);
                    int& owner = block_of[(size_t)(ix - 1) * Ny + (iy - 1)];
                    CHECK(owner == -1);
                    owner = a * my + b;
                }
        }
    CHECK(sum == (long long)(s.ix1 - s.ix0 + 1) * (s.iy1 - s.iy0 + 1));
    for (int ix = 1; ix <= Nx; ++ix)
        for (int iy = 1; iy <= Ny; ++iy) {
            const bool in = ix >= s.ix0 && ix <= s.ix1 && iy >= s.iy0 && iy <= s.iy1;
            CHECK((block_of[(size_t)(ix - 1) * Ny + (iy - 1)] >= 0) == in);
        }
    if (s.reduce == FRAME_MEAN) {
        // k_frame_mean: grid (frame_groups, mx), 256 lanes
        const int nb = frame_group_blocks(s.sy), groups = frame_groups(s);
        CHECK(nb >= 1 && nb * s.sy <= FRAME_THREADS && groups * nb >= my && (groups - 1) * nb < my);
        for (int a = 0; a < mx; ++a)
            for (int g = 0; g < groups; ++g) {
                const int b0 = frame_group_block0(s, g), ncol = frame_group_cols(s, g), rows = frame_block_rows(s, a);
                CHECK(ncol >= 1 && ncol <= FRAME_THREADS);
                std::vector<int> lds((size_t)FRAME_LDS_COLS, 0);
                for (int t = 0; t < FRAME_THREADS; ++t) {
                    if (t >= ncol) continue;
                    const int iy = frame_col0(s, b0) + t;
                    for (int r = 0; r < rows; ++r) cells[(size_t)(frame_row0(s, a) + r - 1) * Ny + (iy - 1)] += 1;
                    CHECK(frame_lds_at(t) >= 0 && frame_lds_at(t) < FRAME_LDS_COLS);
                    lds[(size_t)frame_lds_at(t)] += 1;
                }
                for (int t = 0; t < FRAME_THREADS; ++t) {
                    const int b = b0 + t;
                    if (t >= nb || b >= my) continue;
                    const int cols = frame_block_cols(s, b), first = t * s.sy;
                    for (int c = 0; c < cols; ++c) {
                        CHECK(first + c < ncol);                                    // a column sum some lane wrote
                        CHECK(lds[(size_t)frame_lds_at(first + c)] == 1);           // ... once: no two lanes share a slot
                        // the lane of that slot read the column of block b
                        CHECK(block_of[(size_t)(frame_row0(s, a) - 1) * Ny + (frame_col0(s, b0) + first + c - 1)] == a * my + b);
                    }
                    for (int r = 0; r < nf; ++r) hits[(size_t)frame_at(r, a, b, mx, my)] += 1;
                }
            }
        for (int ix = 1; ix <= Nx; ++ix)
            for (int iy = 1; iy <= Ny; ++iy) {
                const bool in = ix >= s.ix0 && ix <= s.ix1 && iy >= s.iy0 && iy <= s.iy1;
                CHECK(cells[(size_t)(ix - 1) * Ny + (iy - 1)] == (in ? 1 : 0));
            }
    } else {
        // k_frame_sample: grid (ceil(my / 256), mx), one thread per output point
        const int gx = (my + FRAME_THREADS - 1) / FRAME_THREADS;
        for (int a = 0; a < mx; ++a)
            for (int g = 0; g < gx; ++g)
                for (int t = 0; t < FRAME_THREADS; ++t) {
                    const int b = g * FRAME_THREADS + t;
                    if (b >= my) continue;
                    const int ix = frame_row0(s, a), iy = frame_col0(s, b);
                    CHECK(ix >= s.ix0 && ix <= s.ix1 && iy >= s.iy0 && iy <= s.iy1);
                    cells[(size_t)(ix - 1) * Ny + (iy - 1)] += 1;
                    for (int r = 0; r < nf; ++r) hits[(size_t)frame_at(r, a, b, mx, my)] += 1;
                }
        CHECK(std::count(cells.begin(), cells.end(), 1) == (long long)mx * my && std::count(cells.begin(), cells.end(), 0) == (long long)Nx * Ny - (long long)mx * my);
    }
    CHECK(std::count(hits.begin(), hits.end(), 1) == frame_values(s));
}

int main() {
    // the sweep: odd sizes, ragged ends, single rows and columns, strides 1 and 64, windows wider than one workgroup's run
    const int grids[][2] = {{48, 37}, {24, 300}, {100, 1}, {1, 700}, {5, 257}, {3, 1030}};
    const int strides[][2] = {{1, 1}, {2, 2}, {3, 5}, {7, 3}, {64, 64}, {1, 4}, {4, 1}, {2, 3}, {1, 3}, {5, 64}, {64, 1}, {1, 255}, {1, 17}};
    for (const auto& g : grids) {
        const int Nx = g[0], Ny = g[1];
        const int windows[][4] = {{1, Nx, 1, Ny}, {Nx > 4 ? 5 : 1, Nx > 8 ? Nx - 7 : Nx, Ny > 3 ? 4 : 1, Ny > 8 ? Ny - 4 : Ny}, {Nx, Nx, 1, Ny},
                                  {1, Nx, Ny, Ny}, {1, 1, 1, 1}, {1, Nx, Ny > 2 ? 2 : 1, Ny}};
        for (const auto& w : windows)
            for (const auto& st : strides) {
                if (st[0] > FRAME_MAX_STRIDE || st[1] > FRAME_MAX_STRIDE) continue;
                for (int reduce : {FRAME_SAMPLE, FRAME_MEAN})
                    for (int mask : {FRAME_ALL, 0x0f, 0x110}) {
                        FrameSpec s = {mask, w[0], w[1], w[2], w[3], st[0], st[1], reduce, mask == 0x0f};
                        walk(Nx, Ny, s);
                    }
            }
    }
    // 24 x 300 at sy = 3: 85 blocks per workgroup, 255 columns; the 100 blocks take two workgroups, the second 45 columns
    {
        FrameSpec s = {FRAME_ALL, 1, 24, 1, 300, 7, 3, FRAME_MEAN, 0};
        CHECK(frame_group_blocks(3) == 85 && frame_my(s) == 100 && frame_groups(s) == 2 && frame_group_cols(s, 0) == 255 && frame_group_cols(s, 1) == 45);
        CHECK(frame_group_block0(s, 1) == 85 && frame_mx(s) == 4 && frame_block_rows(s, 3) == 3);
    }
    CHECK(frame_group_blocks(1) == 256 && frame_group_blocks(64) == 4 && frame_group_blocks(33) == 7 && frame_group_blocks(5) == 51);
    // the threads that add a block's columns, sy doubles apart, meet in no bank of 32 doubles for the strides a picture uses
    for (int sy : {2, 4, 8, 16}) {
        std::vector<int> bank(32, 0);
        for (int t = 0; t < 32 && t < frame_group_blocks(sy); ++t) bank[(size_t)(frame_lds_at(t * sy) % 32)] += 1;
        CHECK(*std::max_element(bank.begin(), bank.end()) == 1);
    }
    // ranks: the place of a selected field among the selected ones
    CHECK(frame_fields(FRAME_ALL) == 9 && frame_fields(0x0f) == 4 && frame_fields(0x110) == 2 && frame_fields(0) == 0);
    CHECK(frame_rank(FRAME_ALL, 8) == 8 && frame_rank(0x110, 4) == 0 && frame_rank(0x110, 8) == 1 && frame_rank(0x0f, 3) == 3);
    CHECK((FRAME_TAU & FRAME_GAP) == FRAME_TAU && (FRAME_GAP & ~FRAME_TAU) == (1 << 4) && (FRAME_TAU & 0x1f) == 0);
    // what gpf_frames_set accepts
    const FrameSpec ok = {0x0f, 1, 48, 1, 37, 8, 8, FRAME_MEAN, 1};
    CHECK(frame_check(ok, 48, 37) == 0);
    for (int mask : {0, -1, FRAME_ALL + 1, 1 << 9}) { FrameSpec s = ok; s.mask = mask; CHECK(frame_check(s, 48, 37) == 1); }
    for (const auto& w : {std::vector<int>{0, 48, 1, 37}, {1, 49, 1, 37}, {1, 48, 0, 37}, {1, 48, 1, 38}, {9, 3, 1, 37}, {1, 48, 30, 2}}) {
        FrameSpec s = ok; s.ix0 = w[0]; s.ix1 = w[1]; s.iy0 = w[2]; s.iy1 = w[3]; CHECK(frame_check(s, 48, 37) == 2);
    }
    for (const auto& st : {std::vector<int>{0, 1}, {1, 0}, {65, 1}, {1, 65}, {-3, 2}}) { FrameSpec s = ok; s.sx = st[0]; s.sy = st[1]; CHECK(frame_check(s, 48, 37) == 3); }
    for (int r : {-1, 2}) { FrameSpec s = ok; s.reduce = r; CHECK(frame_check(s, 48, 37) == 4); }
    for (int d : {-1, 2}) { FrameSpec s = ok; s.f4 = d; CHECK(frame_check(s, 48, 37) == 5); }
    // a mean over blocks of one cell is stored as a sample; no other stride is
    { FrameSpec s = ok; s.sx = s.sy = 1; frame_normalise(s); CHECK(s.reduce == FRAME_SAMPLE); }
    { FrameSpec s = ok; s.sx = 1; s.sy = 2; frame_normalise(s); CHECK(s.reduce == FRAME_MEAN); s.sx = 2; s.sy = 1; frame_normalise(s); CHECK(s.reduce == FRAME_MEAN); }
    // the headline frame: 4096 x 4096 at (8, 8), four fields, f4 = 4 MiB; sixteen fit the default 64 MiB
    {
        const FrameSpec s = {0x0f, 1, 4096, 1, 4096, 8, 8, FRAME_MEAN, 1};
        CHECK(frame_mx(s) == 512 && frame_my(s) == 512 && frame_record_bytes(s) == 4LL << 20);
        CHECK(frames_default_capacity(64LL << 20, frame_record_bytes(s), 4096, 1) == 16);
        CHECK(frames_default_capacity(64LL << 20, frame_record_bytes(s), 4096, 1000) == 5);
    }
    // default capacity: what fits the budget (a record's bytes rounded up to 8), at least 1, at most ceil(log_cap / every)
    CHECK(frames_default_capacity(64LL << 20, 4, 4096, 1) == 4096 && frames_default_capacity(64LL << 20, 4, 4096, 3) == 1366);
    CHECK(frames_default_capacity(1 << 20, 9LL * 8 * 4096 * 4096, 4096, 1) == 1);
    CHECK(frames_default_capacity(1000, 100, 4096, 1) == 1000 / 104 && frames_default_capacity(1000, 104, 4096, 1) == 1000 / 104);
    for (long long bytes : {4LL, 12LL, 100LL, 4LL << 20})
        for (long long budget : {1000LL, 64LL << 20}) {
            const long long c = frames_default_capacity(budget, bytes, 4096, 1);
            CHECK(c >= 1 && (c == 1 || c * bytes <= budget));
        }
    // the batch limit, replayed as gpf_step's loop: never more than `capacity` records in a batch, every multiple of the stride
    // recorded once, in order, each in the slot of its rank within its batch
    const long long log_cap = 4096;
    for (long long every : {1LL, 3LL, 7LL})
        for (long long capacity : {1LL, 2LL, 5LL, 600LL})
            for (long long start : {0LL, 1LL, 2LL, 6LL, 7LL, 20LL, 4095LL})
                for (long long n : {1LL, 2LL, 7LL, 12LL, 50LL, 9000LL}) {
                    std::vector<long long> recorded;
                    long long done = 0, host_step = start, batches = 0;
                    while (done < n) {
                        const long long base = host_step;
                        const long long limit = frames_batch_limit(base, every, capacity);
                        CHECK(limit >= 1);
                        const long long batch = std::min(std::min(n - done, log_cap), limit);
                        CHECK(batch >= 1);
                        CHECK(lines_count(base, batch, every) <= capacity);
                        std::vector<int> slots((size_t)capacity, 0);
                        for (long long i = 0; i < batch; ++i) {
                            const long long expect = base + i + 1;
                            if (expect % every != 0) continue;
                            const long long slot = lines_count(base, expect - base, every) - 1;
                            CHECK(slot >= 0 && slot < capacity);
                            if (slot >= 0 && slot < capacity) slots[(size_t)slot] += 1;
                            recorded.push_back(expect);
                        }
                        const long long cnt = lines_count(base, batch, every);
                        for (long long k = 0; k < capacity; ++k) CHECK(slots[(size_t)k] == (k < cnt ? 1 : 0));
                        host_step += batch; done += batch; ++batches;
                    }
                    CHECK(host_step == start + n);
                    std::vector<long long> want;
                    for (long long k = start + 1; k <= start + n; ++k) if (k % every == 0) want.push_back(k);
                    CHECK(recorded == want);
                    if (capacity * every >= std::min(n, log_cap) + every) CHECK(batches == (n + log_cap - 1) / log_cap);
                }
    static_assert(sizeof(FrameSpec) == 36, "FrameSpec: nine ints, as gpf_frame_spec");
    std::printf("%s\n", failed ? "FAILED" : "frames.hpp: all checks passed");
    return failed ? 1 : 0;
}
"""


def test_block_and_batch_arithmetic_on_the_host_under_sanitizers(tmp_path):
    cxx = shutil.which('g++')
    if cxx is None:
        pytest.fail("g++ is needed to compile gapflow_amd/csrc/frames.hpp for the host")
    src, exe = tmp_path / 'frames_check.cpp', tmp_path / 'frames_check'
    src.write_text(PROGRAM)
    build = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                            '-static-libasan', '-static-libubsan',      # the runtimes inside the program: it stands alone
                            '-I', os.path.join(ROOT, 'gapflow_amd', 'csrc'), '-o', str(exe), str(src)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'frames.hpp: all checks passed' in run.stdout
