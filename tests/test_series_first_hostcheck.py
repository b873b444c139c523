"""First candidates of the recorded series: the order of gapflow_amd/csrc/series_first.hpp -- extrema_before and FirstAcc (none,
take, merge), the lines every extrema fold on the device is made of -- compiled for the host with a small program of its own (its
own main) under AddressSanitizer and UndefinedBehaviorSanitizer, and run directly.  Outside hipcc the header leaves its device
qualifiers away and gives only those two.  For some hundreds of small candidate sets with many equal values, folding a set left to
right, right to left and as a balanced tree gives one and the same winner for a maximum and for a minimum (both mask bits), and
that winner is the lexicographic first of (value, ix, iy) found by a plain scan written out here.  Nothing of it is loaded into
python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <vector>
#include "series_first.hpp"

static int failed = 0;
#define CHECK(expr) do { if (!(expr)) { std::printf("FAILED line %d: %s\n", __LINE__, #expr); ++failed; } } while (0)

using namespace gpf;

using Acc = FirstAcc<2, 0b10>;          // quantity 0 a maximum, quantity 1 a minimum, fed the same candidates
struct Cand { double v; int ix, iy; };

static uint64_t state = 0x9e3779b97f4a7c15ull;
static unsigned draw(unsigned n) {      // xorshift64*: the sets are the same on every run
    state ^= state >> 12; state ^= state << 25; state ^= state >> 27;
    return (unsigned)((state * 0x2545f4914f6cdd1dull) >> 33) % n;
}

static Acc leaf(const Cand& c) {
    Acc a;
    a.none();
    a.take(0, c.v, c.ix, c.iy);
    a.take(1, c.v, c.ix, c.iy);
    return a;
}

static Acc tree(const std::vector<Cand>& s, size_t lo, size_t hi) {         // [lo, hi), hi > lo
    if (hi - lo == 1) return leaf(s[lo]);
    const size_t mid = lo + (hi - lo) / 2;
    Acc a = tree(s, lo, mid);
    a.merge(tree(s, mid, hi));
    return a;
}

static bool same(const Acc& a, const Acc& b) {
    bool ok = true;
    for (int k = 0; k < 2; ++k) ok = ok && a.v[k] == b.v[k] && a.ix[k] == b.ix[k] && a.iy[k] == b.iy[k];
    return ok;
}

int main() {
    static_assert(Acc::n == 2 && !Acc::is_min(0) && Acc::is_min(1), "mask bit k: quantity k is a minimum");
    // the order itself: the better value, then the smaller ix, then the smaller iy; irreflexive
    CHECK(extrema_before(false, 2., 9, 9, 1., 1, 1) && !extrema_before(false, 1., 1, 1, 2., 9, 9));
    CHECK(extrema_before(true, 1., 9, 9, 2., 1, 1) && !extrema_before(true, 2., 1, 1, 1., 9, 9));
    CHECK(extrema_before(false, 1., 2, 9, 1., 3, 1) && extrema_before(true, 1., 2, 9, 1., 3, 1));
    CHECK(extrema_before(false, 1., 2, 4, 1., 2, 5) && !extrema_before(false, 1., 2, 5, 1., 2, 4));
    CHECK(!extrema_before(false, 1., 2, 4, 1., 2, 4) && !extrema_before(true, 1., 2, 4, 1., 2, 4));
    {   // none(): every cell comes before it, infinities of the wrong sign included
        Acc a;
        a.none();
        CHECK(a.ix[0] == EXTREMA_NO_CELL && a.iy[1] == EXTREMA_NO_CELL);
        a.take(0, -__builtin_huge_val(), 7, 8);
        a.take(1, __builtin_huge_val(), 7, 8);
        CHECK(a.ix[0] == 7 && a.iy[0] == 8 && a.ix[1] == 7 && a.iy[1] == 8);
        Acc b;
        b.none();
        a.merge(b);
        CHECK(a.ix[0] == 7 && a.ix[1] == 7);
    }
    int sets = 0;
    for (int round = 0; round < 400; ++round) {
        const int nx = 1 + (int)draw(5), ny = 1 + (int)draw(7), nvalues = 1 + (int)draw(3);    // few values: many ties
        std::vector<Cand> s;
        for (int ix = 1; ix <= nx; ++ix)
            for (int iy = 1; iy <= ny; ++iy) s.push_back({(double)draw((unsigned)nvalues) - 1., ix, iy});
        for (size_t k = s.size(); k > 1; --k) std::swap(s[k - 1], s[draw((unsigned)k)]);        // the order a fold meets them in is free
        const size_t n = s.size();
        // the lexicographic first of (value, ix, iy), by a plain scan
        Cand best[2] = {s[0], s[0]};
        for (const Cand& c : s) {
            if (c.v > best[0].v || (c.v == best[0].v && (c.ix < best[0].ix || (c.ix == best[0].ix && c.iy < best[0].iy)))) best[0] = c;
            if (c.v < best[1].v || (c.v == best[1].v && (c.ix < best[1].ix || (c.ix == best[1].ix && c.iy < best[1].iy)))) best[1] = c;
        }
        Acc left, right;
        left.none(); right.none();
        for (size_t k = 0; k < n; ++k) { left.merge(leaf(s[k])); right.merge(leaf(s[n - 1 - k])); }
        const Acc balanced = tree(s, 0, n);
        CHECK(same(left, right) && same(left, balanced));
        for (int k = 0; k < 2; ++k) CHECK(left.v[k] == best[k].v && left.ix[k] == best[k].ix && left.iy[k] == best[k].iy);
        ++sets;
    }
    CHECK(sets == 400);
    std::printf("%s\n", failed ? "FAILED" : "series_first.hpp: all checks passed");
    return failed ? 1 : 0;
}
"""


def test_first_candidate_order_on_the_host_under_sanitizers(tmp_path):
    cxx = shutil.which('g++')
    if cxx is None:
        pytest.fail("g++ is needed to compile gapflow_amd/csrc/series_first.hpp for the host")
    src, exe = tmp_path / 'series_first_check.cpp', tmp_path / 'series_first_check'
    src.write_text(PROGRAM)
    build = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-Wno-unknown-pragmas',       # (the header's `#pragma unroll` is the device compiler's)
                            '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                            '-static-libasan', '-static-libubsan',      # the runtimes inside the program: it stands alone
                            '-I', os.path.join(ROOT, 'gapflow_amd', 'csrc'), '-o', str(exe), str(src)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'series_first.hpp: all checks passed' in run.stdout
