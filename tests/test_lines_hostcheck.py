"""Line profiles: the index and order arithmetic of gapflow_amd/csrc/lines.hpp -- the header the device kernels and the library's
argument checks include -- compiled for the host with a small program of its own (its own main) under AddressSanitizer and
UndefinedBehaviorSanitizer, and run directly: where a line's values sit in a record, how a band along y is cut into chunks of 32
rows, the centre line, the checks gpf_lines_set applies, and the capacity / batch-limit arithmetic of gpf_step replayed over whole
runs (never more than `capacity` records in a batch, no recorded step skipped).  Nothing of it is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <algorithm>
#include <cstdio>
#include <vector>
#include "lines.hpp"

static int failed = 0;
#define CHECK(expr) do { if (!(expr)) { std::printf("FAILED line %d: %s\n", __LINE__, #expr); ++failed; } } while (0)

int main() {
    using namespace gpf;
    // record offsets: per line nine fields of `length` doubles, the lines back to back; every index written exactly once
    const int Nx = 45, Ny = 37;
    Line l[4] = {{0, 19, 19, 0, 0, 0}, {1, 1, 45, 0, 0, 0}, {0, 3, 9, 0, 0, 0}, {1, 7, 7, 0, 0, 0}};
    long long scratch = -1;
    const long long rec = lines_layout(l, 4, Nx, Ny, &scratch);
    CHECK(rec == 9LL * (45 + 37 + 45 + 37));
    CHECK(l[0].len == 45 && l[1].len == 37 && l[2].len == 45 && l[3].len == 37);
    CHECK(l[0].rec_off == 0 && l[1].rec_off == 9 * 45 && l[2].rec_off == 9 * (45 + 37) && l[3].rec_off == 9 * (45 + 37 + 45));
    CHECK(line_at(l[0], 0, 0) == 0 && line_at(l[0], 8, 44) == 9 * 45 - 1 && line_at(l[1], 0, 0) == 9 * 45 && line_at(l[3], 8, 36) == rec - 1);
    std::vector<int> hits((size_t)rec, 0);      // (the vector is what the sanitizer watches the indices on)
    for (int k = 0; k < 4; ++k)
        for (int f = 0; f < LINE_NF; ++f)
            for (int j = 0; j < l[k].len; ++j) hits[(size_t)line_at(l[k], f, j)] += 1;
    CHECK(std::count(hits.begin(), hits.end(), 1) == rec);
    CHECK(line_at(l[2], 3, 10) == l[2].rec_off + 3 * 45 + 10);
    // only the band along y needs scratch: [chunks][9][Ny], 45 rows = 2 chunks
    CHECK(scratch == 2LL * 9 * 37);
    CHECK(l[1].scratch_off == 0 && line_scratch_doubles(l[0]) == 0 && line_scratch_doubles(l[2]) == 0 && line_scratch_doubles(l[3]) == 0);
    CHECK(line_is_band(l[1]) && line_is_band(l[2]) && !line_is_band(l[0]) && !line_is_band(l[3]));
    CHECK(line_band_cells(l[1]) == 45 && line_band_cells(l[2]) == 7 && line_band_cells(l[0]) == 1);
    // chunk counts: exactly 32 rows, 33 rows, 1 row (and the 32 + 13 of 45); the chunks' rows add up to the band
    CHECK(line_chunks(32) == 1 && line_chunk_rows(32, 0) == 32);
    CHECK(line_chunks(33) == 2 && line_chunk_rows(33, 0) == 32 && line_chunk_rows(33, 1) == 1);
    CHECK(line_chunks(1) == 1 && line_chunk_rows(1, 0) == 1);
    CHECK(line_chunks(45) == 2 && line_chunk_rows(45, 0) == 32 && line_chunk_rows(45, 1) == 13);
    CHECK(line_chunks(64) == 2 && line_chunk_rows(64, 1) == 32 && line_chunks(65) == 3 && line_chunks(4096) == 128);
    for (int n = 1; n <= 200; ++n) {
        int sum = 0;
        for (int c = 0; c < line_chunks(n); ++c) { CHECK(line_chunk_rows(n, c) >= 1 && line_chunk_rows(n, c) <= LINE_CHUNK); sum += line_chunk_rows(n, c); }
        CHECK(sum == n);
    }
    // the centre line: ny // 2 of the ghosted shape
    CHECK(line_centre(0, 45, 37) == 19 && line_centre(1, 45, 37) == 23 && line_centre(0, 100, 1) == 1 && line_centre(1, 100, 1) == 51);
    CHECK(line_centre(0, 20, 70) == 36 && line_centre(1, 20, 70) == 11 && line_centre(0, 8, 2) == 2 && line_centre(1, 1, 8) == 1);
    for (int n = 1; n <= 50; ++n) CHECK(line_centre(0, 3, n) >= 1 && line_centre(0, 3, n) <= n && line_centre(0, 3, n) == (n + 2) / 2);
    CHECK(line_length(0, 45, 37) == 45 && line_length(1, 45, 37) == 37);
    // what gpf_lines_set accepts: along x the indices are columns (1..Ny), along y rows (1..Nx)
    CHECK(line_check(0, 1, 37, Nx, Ny) == 0 && line_check(1, 1, 45, Nx, Ny) == 0 && line_check(0, 37, 37, Nx, Ny) == 0);
    CHECK(line_check(2, 1, 1, Nx, Ny) == 1 && line_check(-1, 1, 1, Nx, Ny) == 1);
    CHECK(line_check(0, 0, 5, Nx, Ny) == 2 && line_check(0, 1, 38, Nx, Ny) == 2 && line_check(0, 9, 3, Nx, Ny) == 2);
    CHECK(line_check(1, 1, 46, Nx, Ny) == 2 && line_check(1, 38, 45, Nx, Ny) == 0 && line_check(1, 0, 0, Nx, Ny) == 2);
    // default capacity: what fits the budget, at least 1, at most ceil(log_cap / every)
    CHECK(lines_default_capacity(64LL << 20, 9 * 4096, 4096, 1) == (64LL << 20) / (9 * 4096 * 8));
    CHECK(lines_default_capacity(64LL << 20, 9 * 100, 4096, 1) == 4096 && lines_default_capacity(64LL << 20, 9 * 100, 4096, 3) == 1366);
    CHECK(lines_default_capacity(64LL << 20, 9 * 100, 4096, 5000) == 1);
    CHECK(lines_default_capacity(1 << 20, 8LL * 9 * 46000, 4096, 1) == 1);
    // the batch limit, replayed as gpf_step's loop: never more than `capacity` records in a batch, every multiple of the stride
    // recorded once, in order, each in the slot of its rank within its batch
    const long long log_cap = 4096;
    for (long long every : {1LL, 3LL, 7LL})
        for (long long capacity : {1LL, 2LL, 5LL, 600LL})
            for (long long start : {0LL, 1LL, 2LL, 6LL, 7LL, 20LL, 4095LL})
                for (long long n : {1LL, 2LL, 12LL, 50LL, 9000LL}) {
                    std::vector<long long> recorded;
                    long long done = 0, host_step = start, batches = 0;
                    while (done < n) {
                        const long long base = host_step;
                        const long long limit = lines_batch_limit(base, every, capacity);
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
                        for (long long s = 0; s < capacity; ++s) CHECK(slots[(size_t)s] == (s < cnt ? 1 : 0));
                        host_step += batch; done += batch; ++batches;
                    }
                    CHECK(host_step == start + n);
                    std::vector<long long> want;
                    for (long long s = start + 1; s <= start + n; ++s) if (s % every == 0) want.push_back(s);
                    CHECK(recorded == want);
                    // a capacity that holds the whole call's records does not add batches
                    if (capacity * every >= std::min(n, log_cap) + every) CHECK(batches == (n + log_cap - 1) / log_cap);
                }
    static_assert(sizeof(Line) == 32, "Line: four ints and two 64-bit offsets");
    std::printf("%s\n", failed ? "FAILED" : "lines.hpp: all checks passed");
    return failed ? 1 : 0;
}
"""


def test_index_and_batch_arithmetic_on_the_host_under_sanitizers(tmp_path):
    cxx = shutil.which('g++')
    if cxx is None:
        pytest.fail("g++ is needed to compile gapflow_amd/csrc/lines.hpp for the host")
    src, exe = tmp_path / 'lines_check.cpp', tmp_path / 'lines_check'
    src.write_text(PROGRAM)
    build = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                            '-static-libasan', '-static-libubsan',      # the runtimes inside the program: it stands alone
                            '-I', os.path.join(ROOT, 'gapflow_amd', 'csrc'), '-o', str(exe), str(src)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'lines.hpp: all checks passed' in run.stdout
