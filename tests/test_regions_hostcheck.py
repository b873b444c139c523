"""Region series: the membership rules of gapflow_amd/csrc/regions.hpp -- the header the device kernels include -- compiled for the
host with a small program of its own (its own main) under AddressSanitizer and UndefinedBehaviorSanitizer, and run directly: a
value equal to lo (in), equal to hi (out), -0.0 against a bound of 0.0, infinite bounds, NaN (out), the box edges, and the checks
gpf_regions_set applies to a region.  Nothing of it is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <limits>
#include "regions.hpp"

static int failed = 0;
#define CHECK(expr) do { if (!(expr)) { std::printf("FAILED line %d: %s\n", __LINE__, #expr); ++failed; } } while (0)

int main() {
    using namespace gpf;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double big = std::numeric_limits<double>::max(), tiny = std::numeric_limits<double>::denorm_min();
    // lo is inclusive, hi exclusive
    CHECK(region_value_in(2.0, 2.0, 3.0));
    CHECK(!region_value_in(3.0, 2.0, 3.0));
    CHECK(region_value_in(std::nextafter(3.0, 0.0), 2.0, 3.0));
    CHECK(!region_value_in(std::nextafter(2.0, 0.0), 2.0, 3.0));
    // -0.0 equals 0.0: it belongs to [0, hi) and not to [lo, 0)
    CHECK(region_value_in(-0.0, 0.0, 1.0));
    CHECK(region_value_in(0.0, -0.0, 1.0));
    CHECK(!region_value_in(-0.0, -1.0, 0.0));
    CHECK(!region_value_in(0.0, -1.0, -0.0));
    CHECK(region_value_in(-tiny, -1.0, 0.0));
    CHECK(!region_value_in(-tiny, 0.0, 1.0));
    // infinite bounds leave a side open; +inf itself is never below hi = +inf, -inf belongs to lo = -inf
    CHECK(region_value_in(-big, -inf, 0.0));
    CHECK(region_value_in(big, 0.0, inf));
    CHECK(region_value_in(0.0, -inf, inf));
    CHECK(region_value_in(-inf, -inf, inf));
    CHECK(!region_value_in(inf, -inf, inf));
    CHECK(!region_value_in(inf, 0.0, inf));
    // a NaN never belongs
    CHECK(!region_value_in(nan, -inf, inf));
    CHECK(!region_value_in(nan, 0.0, 1.0));
    CHECK(!region_value_in(1.0, nan, 2.0));
    CHECK(!region_value_in(1.0, 0.0, nan));
    // the box: inclusive on all four edges
    for (int ix = 0; ix <= 9; ++ix)
        for (int iy = 0; iy <= 9; ++iy)
            CHECK(region_box_in(ix, iy, 3, 5, 2, 7) == (ix >= 3 && ix <= 5 && iy >= 2 && iy <= 7));
    CHECK(region_box_in(3, 2, 3, 5, 2, 7) && region_box_in(5, 7, 3, 5, 2, 7) && region_box_in(3, 7, 3, 5, 2, 7) && region_box_in(5, 2, 3, 5, 2, 7));
    CHECK(!region_box_in(2, 2, 3, 5, 2, 7) && !region_box_in(6, 7, 3, 5, 2, 7) && !region_box_in(3, 1, 3, 5, 2, 7) && !region_box_in(5, 8, 3, 5, 2, 7));
    CHECK(region_box_in(4, 4, 4, 4, 4, 4) && !region_box_in(4, 5, 4, 4, 4, 4));
    // both together, as the kernel asks
    Region r;
    r.lo = 1.0; r.hi = inf; r.field = 1; r.ix0 = 1; r.ix1 = 8; r.iy0 = 2; r.iy1 = 2; r.pad_ = 0;
    CHECK(region_member(r, 1.0, 1, 2) && region_member(r, big, 8, 2));
    CHECK(!region_member(r, 1.0, 1, 3) && !region_member(r, 0.5, 1, 2) && !region_member(r, nan, 1, 2) && !region_member(r, 1.0, 9, 2));
    // what gpf_regions_set accepts
    CHECK(region_check(0, -inf, inf, 1, 8, 1, 6, 8, 6) == 0);
    CHECK(region_check(4, 0.0, tiny, 8, 8, 6, 6, 8, 6) == 0);
    CHECK(region_check(-1, 0.0, 1.0, 1, 8, 1, 6, 8, 6) == 1 && region_check(REGION_NFIELD, 0.0, 1.0, 1, 8, 1, 6, 8, 6) == 1);
    CHECK(region_check(1, 1.0, 1.0, 1, 8, 1, 6, 8, 6) == 2 && region_check(1, 2.0, 1.0, 1, 8, 1, 6, 8, 6) == 2);
    CHECK(region_check(1, nan, 1.0, 1, 8, 1, 6, 8, 6) == 2 && region_check(1, 0.0, nan, 1, 8, 1, 6, 8, 6) == 2);
    CHECK(region_check(1, inf, inf, 1, 8, 1, 6, 8, 6) == 2 && region_check(1, 0.0, -0.0, 1, 8, 1, 6, 8, 6) == 2);
    CHECK(region_check(1, 0.0, 1.0, 0, 8, 1, 6, 8, 6) == 3 && region_check(1, 0.0, 1.0, 1, 9, 1, 6, 8, 6) == 3);
    CHECK(region_check(1, 0.0, 1.0, 1, 8, 0, 6, 8, 6) == 3 && region_check(1, 0.0, 1.0, 1, 8, 1, 7, 8, 6) == 3);
    CHECK(region_check(1, 0.0, 1.0, 5, 4, 1, 6, 8, 6) == 3 && region_check(1, 0.0, 1.0, 1, 8, 4, 3, 8, 6) == 3);
    static_assert(sizeof(Region) == 40, "Region: two doubles and six ints");
    std::printf("%s\n", failed ? "FAILED" : "regions.hpp: all checks passed");
    return failed ? 1 : 0;
}
"""


def test_predicate_header_on_the_host_under_sanitizers(tmp_path):
    cxx = shutil.which('g++')
    if cxx is None:
        pytest.fail("g++ is needed to compile gapflow_amd/csrc/regions.hpp for the host")
    src, exe = tmp_path / 'regions_check.cpp', tmp_path / 'regions_check'
    src.write_text(PROGRAM)
    build = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                            '-static-libasan', '-static-libubsan',      # the runtimes inside the program: it stands alone
                            '-I', os.path.join(ROOT, 'gapflow_amd', 'csrc'), '-o', str(exe), str(src)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'regions.hpp: all checks passed' in run.stdout
