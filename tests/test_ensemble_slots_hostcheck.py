"""Ensemble series: the slot arithmetic of gapflow_amd/csrc/ensemble_slots.hpp -- the one place that says where a member's records
of a series lie inside that series' device allocation -- compiled for the host with a small program of its own (its own main) under
AddressSanitizer and UndefinedBehaviorSanitizer, and run directly.  Over a sweep of member counts, strides, film widths and probe
counts, for the three layouts gpf_ensemble_*_set build: every member's region of every channel lies inside the total, no two
regions overlap, channels of doubles start on 8 bytes and channels of int32 on 4, and the extrema's offsets are the formulas the
library used before the header existed, written out here.  Nothing of it is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <algorithm>
#include <cstdio>
#include <utility>
#include <vector>
#include "ensemble_slots.hpp"

static int failed = 0;
#define CHECK(expr) do { if (!(expr)) { std::printf("FAILED line %d: %s\n", __LINE__, #expr); ++failed; } } while (0)

using namespace gpf;

constexpr long long LOG_CAPACITY = 4096;
constexpr int FILM_NSUM = 9, EXTREMA_NQ = 7;

// What holds for every layout: `align[c]` is the size of channel c's values.  Every byte of the allocation is counted in `owner`
// (the vector is what the sanitizer watches): regions inside the total, apart, and together the whole of it.
static void check(const EnsembleSlots& s, const std::vector<std::vector<size_t>>& record_bytes, const std::vector<long long>& cap,
                  const std::vector<size_t>& align) {
    const int m = (int)cap.size(), channels = (int)record_bytes.size();
    CHECK(s.m == m && s.off.size() == (size_t)m * channels && s.bytes.size() == s.off.size());
    std::vector<std::pair<size_t, size_t>> regions;
    size_t sum = 0;
    for (int c = 0; c < channels; ++c)
        for (int i = 0; i < m; ++i) {
            const size_t begin = s.at(c, i), bytes = (size_t)cap[(size_t)i] * record_bytes[(size_t)c][(size_t)i];
            CHECK(s.record_bytes(c, i) == record_bytes[(size_t)c][(size_t)i]);
            CHECK(bytes > 0 && begin + bytes <= s.total);
            CHECK(begin % align[(size_t)c] == 0);
            regions.push_back({begin, begin + bytes});
            sum += bytes;
        }
    CHECK(sum == s.total);
    std::sort(regions.begin(), regions.end());
    for (size_t k = 1; k < regions.size(); ++k) CHECK(regions[k - 1].second <= regions[k].first);
    if (s.total <= (size_t)1 << 22) {           // (the larger ones stand on the sorted comparison above)
        std::vector<unsigned char> owner(s.total, 0);
        for (const auto& r : regions)
            for (size_t b = r.first; b < r.second; ++b) owner[b] += 1;
        CHECK(std::count(owner.begin(), owner.end(), 1) == (long long)s.total);
    }
}

int main() {
    const long long everys[] = {1, 3, 4096, 4097}, caps[] = {4097, 1366, 2, 1};
    for (int m : {1, 2, 3, 17})
        for (int e = 0; e < 4; ++e) {
            const long long every = everys[e], cap = LOG_CAPACITY / every + 1;
            CHECK(cap == caps[e]);
            const std::vector<long long> same((size_t)m, cap);
            // film integrals: FILM_NSUM + nsx + nsy doubles, 1 .. 8 sections per direction, mixed across the members
            for (int shift = 0; shift < 8; ++shift) {
                std::vector<size_t> width((size_t)m);
                for (int i = 0; i < m; ++i) width[(size_t)i] = (size_t)(FILM_NSUM + 1 + (i + shift) % 8 + 1 + (3 * i + shift) % 8) * sizeof(double);
                const EnsembleSlots s = ensemble_slots({width}, same);
                check(s, {width}, same, {8});
                size_t doubles = 0;         // members back to back, as gpf_ensemble_integrals_set counted them: in doubles
                for (int i = 0; i < m; ++i) {
                    CHECK(s.at(0, i) == doubles * sizeof(double));
                    doubles += (size_t)cap * (width[(size_t)i] / sizeof(double));
                }
                CHECK(s.total == doubles * sizeof(double));
            }
            for (size_t w : {(size_t)(FILM_NSUM + 1 + 1), (size_t)(FILM_NSUM + 8 + 8)}) {
                const std::vector<size_t> width((size_t)m, w * sizeof(double));
                check(ensemble_slots({width}, same), {width}, same, {8});
            }
            // extrema: all members' values ([m][cap][7] doubles), then all members' cells ([m][cap][7][2] int32)
            {
                const std::vector<std::vector<size_t>> rb = {std::vector<size_t>((size_t)m, EXTREMA_NQ * sizeof(double)),
                                                             std::vector<size_t>((size_t)m, 2 * EXTREMA_NQ * sizeof(int))};
                const EnsembleSlots s = ensemble_slots(rb, same);
                check(s, rb, same, {8, 4});
                // the formulas the library held: val(i) = (double*)rec + i * cap * 7;
                // cell(m, i) = (int*)((double*)rec + m * cap * 7) + i * cap * 2 * 7; the allocation m * cap * 7 * (8 + 2 * 4) bytes
                for (int i = 0; i < m; ++i) {
                    CHECK(s.at(0, i) == ((size_t)i * (size_t)cap * EXTREMA_NQ) * sizeof(double));
                    CHECK(s.at(1, i) == ((size_t)m * (size_t)cap * EXTREMA_NQ) * sizeof(double) + ((size_t)i * (size_t)cap * 2 * EXTREMA_NQ) * sizeof(int));
                }
                CHECK(s.total == (size_t)m * ((size_t)cap * EXTREMA_NQ) * (sizeof(double) + 2 * sizeof(int)));
            }
        }
    // probes: n_i x nv doubles per record, a record per step of the longest call (every member's log capacity)
    const int counts[] = {1, 7, 256};
    for (int m : {1, 2, 3, 17})
        for (int nv : {3, 4})
            for (int shift = 0; shift < 3; ++shift) {
                std::vector<size_t> width((size_t)m);
                for (int i = 0; i < m; ++i) width[(size_t)i] = (size_t)counts[(i + shift) % 3] * (size_t)nv * sizeof(double);
                const std::vector<long long> cap((size_t)m, LOG_CAPACITY);
                const EnsembleSlots s = ensemble_slots({width}, cap);
                check(s, {width}, cap, {8});
                size_t doubles = 0;         // as gpf_ensemble_probes_set counted them
                for (int i = 0; i < m; ++i) {
                    CHECK(s.at(0, i) == doubles * sizeof(double));
                    doubles += (size_t)LOG_CAPACITY * (size_t)counts[(i + shift) % 3] * (size_t)nv;
                }
                CHECK(s.total == doubles * sizeof(double));
            }
    // capacities that differ between the members
    {
        const std::vector<size_t> width = {24, 56, 8};
        const std::vector<long long> cap = {5, 1, 4096};
        const EnsembleSlots s = ensemble_slots({width}, cap);
        check(s, {width}, cap, {8});
        CHECK(s.at(0, 0) == 0 && s.at(0, 1) == 120 && s.at(0, 2) == 176 && s.total == 176 + 8 * 4096);
    }
    std::printf("%s\n", failed ? "FAILED" : "ensemble_slots.hpp: all checks passed");
    return failed ? 1 : 0;
}
"""


def test_slot_arithmetic_on_the_host_under_sanitizers(tmp_path):
    cxx = shutil.which('g++')
    if cxx is None:
        pytest.fail("g++ is needed to compile gapflow_amd/csrc/ensemble_slots.hpp for the host")
    src, exe = tmp_path / 'ensemble_slots_check.cpp', tmp_path / 'ensemble_slots_check'
    src.write_text(PROGRAM)
    build = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                            '-static-libasan', '-static-libubsan',      # the runtimes inside the program: it stands alone
                            '-I', os.path.join(ROOT, 'gapflow_amd', 'csrc'), '-o', str(exe), str(src)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'ensemble_slots.hpp: all checks passed' in run.stdout
