"""Workspace tier of the ensembles: the layout of gapflow_amd/csrc/mid_layout.hpp -- the header the kernel and the library
include -- compiled for the host with a small program of its own (its own main) under AddressSanitizer and
UndefinedBehaviorSanitizer, and run directly.  For 39 x 28 (the first shape beyond LDS), 50 x 50, 20 x 270 (long and narrow) and
126 x 126 (the largest) it allocates exactly the header's byte count, writes the first and the last cell of all 19 planes (a
plane that reached past the allocation would trip the sanitizer) and checks that the planes do not overlap: every tag reads back,
offsets ascend by whole planes.  Nothing of it is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "mid_layout.hpp"

static int failed = 0;
#define CHECK(expr) do { if (!(expr)) { std::printf("FAILED line %d: %s\n", __LINE__, #expr); ++failed; } } while (0)

static void shape(int Nx, int Ny) {
    using namespace gpf;
    const long long nc = mid_cells(Nx, Ny), bytes = mid_workspace_bytes(nc);
    CHECK(nc == (long long)(Nx + 2) * (Ny + 2) && nc <= MID_GRID_MAX_CELLS);
    CHECK(bytes % MID_WORKSPACE_ALIGN == 0 && bytes >= 19 * 8 * nc && bytes < 19 * 8 * nc + MID_WORKSPACE_ALIGN);
    char* raw = (char*)std::malloc((size_t)bytes);          // exactly the header's count: one byte beyond is the sanitizer's
    double* ws = (double*)raw;
    for (int p = 0; p < MID_DOUBLES_PER_CELL; ++p) {
        double* plane = ws + mid_plane_offset(p, nc);
        plane[0] = 2.0 * p + 1.0;
        plane[nc - 1] = -(2.0 * p + 1.0);
    }
    for (int p = 0; p < MID_DOUBLES_PER_CELL; ++p) {        // nobody's first or last cell was anybody else's
        const double* plane = ws + mid_plane_offset(p, nc);
        CHECK(plane[0] == 2.0 * p + 1.0 && plane[nc - 1] == -(2.0 * p + 1.0));
        if (p > 0) CHECK(mid_plane_offset(p, nc) - mid_plane_offset(p - 1, nc) == nc);
        CHECK((char*)(plane + nc) <= raw + bytes);
    }
    CHECK(mid_plane_offset(0, nc) == 0);
    std::free(raw);
}

int main() {
    using namespace gpf;
    static_assert(MID_DOUBLES_PER_CELL == 19 && MID_GRID_MAX_CELLS == 16384 && MID_THREADS == 512, "the limits gapflow_amd/_lib.py states");
    static_assert(MID_PLANE_Q == 0 && MID_PLANE_F == 9 && MID_PLANE_T == 15, "three state buffers, six fluxes and sources, h hx hy Ls");
    shape(39, 28);
    shape(50, 50);
    shape(20, 270);
    shape(126, 126);
    CHECK(mid_cells(126, 126) == MID_GRID_MAX_CELLS && mid_cells(127, 126) > MID_GRID_MAX_CELLS);
    CHECK(mid_workspace_bytes(1) == 256 && mid_workspace_bytes(32) == 19 * 256 && mid_workspace_bytes(33) == 19 * 264 + 104);
    std::printf("%s\n", failed ? "FAILED" : "mid_layout.hpp: all checks passed");
    return failed ? 1 : 0;
}
"""


def test_workspace_layout_on_the_host_under_sanitizers(tmp_path):
    cxx = shutil.which('g++')
    if cxx is None:
        pytest.fail("g++ is needed to compile gapflow_amd/csrc/mid_layout.hpp for the host")
    src, exe = tmp_path / 'mid_layout_check.cpp', tmp_path / 'mid_layout_check'
    src.write_text(PROGRAM)
    build = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                            '-static-libasan', '-static-libubsan',      # the runtimes inside the program: it stands alone
                            '-I', os.path.join(ROOT, 'gapflow_amd', 'csrc'), '-o', str(exe), str(src)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'mid_layout.hpp: all checks passed' in run.stdout
