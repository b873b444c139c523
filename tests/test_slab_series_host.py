"""Domain series on x-slabs, host side -- no GPU: the row map of gapflow_amd/csrc/slab_rows.hpp (the header the fold kernels and
the library's argument checks include) compiled into a small program of its own under the sanitizers and held against
slab.partition; the due-step and slot arithmetic of an advance that the record buffers split; options.domain_series read from the
YAML text; the entry points in the header, the ctypes table and the built library; the old refusals, still in place.  The device
side: tests/test_gpu_slab_series.py."""
import ctypes
import io
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "slab_rows.hpp"

// per (Nx, world): "Nx world max_nx" and per global row "rank local gathered_row", per rank "row0 nx check"
int main() {
    using namespace gpf;
    std::vector<std::pair<int, int>> cases;
    for (int world = 1; world <= 9; ++world)
        for (int Nx = world; Nx <= 40; ++Nx) cases.push_back({Nx, world});
    cases.push_back({4096, 8});
    cases.push_back({523, 8});
    for (auto [Nx, world] : cases) {
        std::printf("C %d %d %d\n", Nx, world, slab_max_nx(Nx, world));
        std::vector<int> hit((size_t)world * slab_max_nx(Nx, world), 0);        // (the vector is what the sanitizer watches the rows on)
        for (int g = 0; g < Nx; ++g) {
            const SlabRow r = slab_row_of(g, Nx, world);
            const long long at = slab_gathered_row(g, Nx, world);
            hit[(size_t)at] += 1;
            std::printf("G %d %d %lld\n", r.rank, r.local, at);
        }
        for (int v : hit) if (v > 1) { std::printf("FAILED: a gathered row is used twice\n"); return 1; }
        for (int r = 0; r < world; ++r) {
            const int row0 = slab_rank_row0(Nx, world, r), nx = slab_rank_nx(Nx, world, r);
            std::printf("R %d %d %d %d %d\n", row0, nx, slab_check(row0, nx, Nx, world), slab_check(row0 + 1, nx, Nx, world),
                        slab_check(row0, nx + 1, Nx, world));
        }
    }
    std::printf("X %d %d %d\n", slab_check(0, 4, 3, 4), slab_check(0, 4, 4, 0), slab_check(-1, 4, 8, 2));
    return 0;
}
"""


def test_row_map_against_partition_on_the_host_under_sanitizers(tmp_path):
    from gapflow_amd.slab import partition
    cxx = shutil.which('g++')
    if cxx is None:
        pytest.fail("g++ is needed to compile gapflow_amd/csrc/slab_rows.hpp for the host")
    src, exe = tmp_path / 'slab_rows_check.cpp', tmp_path / 'slab_rows_check'
    src.write_text(PROGRAM)
    build = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                            '-static-libasan', '-static-libubsan',      # the runtimes inside the program: it stands alone
                            '-I', os.path.join(ROOT, 'gapflow_amd', 'csrc'), '-o', str(exe), str(src)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = iter(run.stdout.splitlines())
    cases = [(nx, w) for w in range(1, 10) for nx in range(w, 41)] + [(4096, 8), (523, 8)]
    for Nx, world in cases:
        parts = partition(Nx, world)
        max_nx = max(hi - lo + 1 for lo, hi in parts)
        assert next(lines) == f"C {Nx} {world} {max_nx}"
        for r, (lo, hi) in enumerate(parts):
            for g in range(lo - 1, hi):                 # global row g (0-based) is rank r's local row g - (lo - 1)
                assert next(lines) == f"G {r} {g - (lo - 1)} {r * max_nx + g - (lo - 1)}", (Nx, world, g)
        for r, (lo, hi) in enumerate(parts):
            nx = hi - lo + 1
            # a slab that starts one row later, or is one row longer, is no rank's -- unless that happens to be the next cut
            shifted = 0 if any(p == (lo + 1, lo + nx) for p in parts) else 2
            longer = 0 if any(p == (lo, lo + nx) for p in parts) else 2
            assert next(lines) == f"R {lo - 1} {nx} 0 {shifted} {longer}", (Nx, world, r)
    assert next(lines) == "X 1 1 2"
    assert next(lines, None) is None


@pytest.mark.parametrize('strides', [(1, 0), (0, 1), (1, 3), (3, 7), (5000, 2)])
def test_due_steps_and_slots_of_an_advance_split_by_the_buffer(strides):
    """SlabDriver._recording replayed on the host: pieces of _domain_chunk steps, each beginning at the count the piece before
    ended on.  No piece leaves more than `cap` records of a series, every due step is recorded once, in order, in the slot of its
    rank among its piece's records (the library's series_slot), and a cap that holds the whole call does not split it."""
    from gapflow_amd.series import _domain_chunk, _integral_records
    for cap in (1, 2, 5, 4096):
        for start in (0, 1, 6, 7, 20, 4095):
            for n in (1, 2, 13, 50, 9000):
                recorded = {every: [] for every in strides if every}
                base, done, pieces = start, 0, 0
                while done < n:
                    piece = _domain_chunk(base, n - done, strides, cap)
                    assert 1 <= piece <= n - done
                    for every in recorded:
                        count = _integral_records(base, piece, every)
                        assert count <= cap
                        slots = []
                        for expect in range(base + 1, base + piece + 1):
                            if expect % every == 0:             # _DomainSeries.due, per series
                                slots.append(_integral_records(base, expect - base, every) - 1)
                                recorded[every].append(expect)
                        assert slots == list(range(count))
                        if piece < n - done:                    # the piece is as long as the fullest buffer allows
                            assert any(_integral_records(base, piece + 1, e) > cap for e in recorded)
                    base, done, pieces = base + piece, done + piece, pieces + 1
                for every, steps in recorded.items():
                    assert steps == [s for s in range(start + 1, start + n + 1) if s % every == 0]
                if all(_integral_records(start, n, e) <= cap for e in recorded):
                    assert pieces == 1


BASE = """
options: {{silent: True{more}}}
grid: {{Nx: 100, Ny: 6, Lx: 0.1, Ly: 1., xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P']}}
geometry: {{type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.}}
numerics: {{CFL: 0.25, adaptive: 1, tol: 1e-12, dt: 1e-10, max_it: 100}}
properties: {{shear: 0.0794, bulk: 0., EOS: DH, P0: 101325., rho0: 877.7007, C1: 3.5e10, C2: 1.23}}
"""


def parsed(more):
    from gapflow_amd.io import read_yaml_input
    from gapflow_amd.problem import _keep_own_options
    text = BASE.format(more=more)
    d = read_yaml_input(io.StringIO(text))
    _keep_own_options(d, text)
    return d


def test_domain_series_is_read_from_the_yaml_text():
    d = parsed(", domain_series: {integrals: 5, extrema: 2, sections_x: [1, 50, 100], sections_y: [3]}")
    assert d['options']['domain_series'] == {'integrals': 5, 'extrema': 2, 'sections_x': [1, 50, 100], 'sections_y': [3]}
    d = parsed(", domain_series: {extrema: 4}")
    assert d['options']['domain_series'] == {'integrals': 0, 'extrema': 4, 'sections_x': None, 'sections_y': None}
    assert 'domain_series' not in parsed("")['options']
    # one of the family at a time, like the other keys
    from gapflow_amd.io import read_yaml_input
    from gapflow_amd.problem import _keep_domain_series
    text = BASE.format(more=", domain_series: {integrals: 1}, integrals: 3")
    d = read_yaml_input(io.StringIO(text))
    _keep_domain_series(d, text)
    assert d['options']['domain_series']['integrals'] == 1 and 'integrals' not in d['options']


@pytest.mark.parametrize('bad,message', [
    ("{integrals: -3}", 'integrals: the stride'), ("{integrals: 1.5}", 'integrals: the stride'), ("{integrals: True}", 'integrals: the stride'),
    ("{integrals: [1]}", 'integrals: the stride'), ("{extrema: -1}", 'extrema: the stride'), ("{extrema: 'often'}", 'extrema: the stride'),
    ("{integrals: 1, sections_x: []}", 'integrals: sections_x'), ("{integrals: 1, sections_x: [0]}", r'sections_x\[0\] = 0 lies outside the interior 1\.\.100'),
    ("{integrals: 1, sections_x: [101]}", r'sections_x\[0\] = 101 lies outside'), ("{integrals: 1, sections_y: [7]}", r'sections_y\[0\] = 7 lies outside the interior 1\.\.6'),
    ("{integrals: 1, sections_y: [1.5]}", r'sections_y\[0\] must be an integer'), ("{integrals: 1, sections_x: [1, 2, 3, 4, 5, 6, 7, 8, 9]}", '9 sections'),
    ("{integrals: 1, every: 2}", 'options.domain_series: a mapping with the keys'), ("4", 'options.domain_series: a mapping with the keys')])
def test_bad_strides_and_sections_raise_with_the_film_integrals_messages(bad, message):
    with pytest.raises(ValueError, match=message):
        parsed(f", domain_series: {bad}")


def test_entry_points_are_declared_bound_and_exported():
    from gapflow_amd import _lib
    from gapflow_amd.build import build_library
    names = ['gpf_slab_series_set', 'gpf_slab_series_clear', 'gpf_slab_series_message', 'gpf_slab_series_begin', 'gpf_slab_series_local',
             'gpf_slab_series_fold', 'gpf_slab_series_end', 'gpf_slab_series_read', 'gpf_slab_series_now_local', 'gpf_slab_series_now_fold']
    with open(os.path.join(ROOT, 'include', 'gapflow_hip.h')) as f:
        header = f.read()
    lib = ctypes.CDLL(build_library())
    for name in names:
        assert re.search(rf'^int {name}\(gpf_handle\* h', header, re.M), f"{name} is not declared in include/gapflow_hip.h"
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and argtypes[0] is ctypes.c_void_p
        fn = getattr(lib, name)                     # exported
        fn.restype, fn.argtypes = restype, argtypes
        args = [None] + [0 if a in (ctypes.c_int, ctypes.c_int64, ctypes.c_size_t) else None for a in argtypes[1:]]
        assert fn(*args) == -1, f"{name}(NULL, ...) must return GPF_ERR_INVALID"     # no device is touched for a null handle
    assert re.search(r'GPF_ERR_INVALID\s*=\s*-1\b', header)
    assert len(_lib.SIGNATURES['gpf_slab_series_set'][1]) == 10 and len(_lib.SIGNATURES['gpf_slab_series_read'][1]) == 8


def test_the_old_names_keep_refusing_and_the_new_calls_exist():
    from gapflow_amd.slab import SlabProblem
    with pytest.raises(NotImplementedError, match='integrals: not available on a SlabProblem'):
        SlabProblem.set_integrals(object(), every=2)
    with pytest.raises(NotImplementedError, match='set_domain_series'):
        SlabProblem.film_integrals(object())
    with pytest.raises(NotImplementedError, match='extrema: not available on a SlabProblem'):
        SlabProblem.set_extrema(object(), every=2)
    with pytest.raises(NotImplementedError, match='integrals: not available on a SlabProblem'):
        SlabProblem.from_string(BASE.format(more=", integrals: 4"), device=0, dist=object())
    with pytest.raises(NotImplementedError, match='extrema: not available on a SlabProblem'):
        SlabProblem.from_string(BASE.format(more=", extrema: 4, domain_series: {integrals: 1}"), device=0, dist=object())
    for name in ('set_domain_series', 'clear_domain_series', 'domain_integrals', 'domain_extrema', 'domain_film_integrals', 'domain_field_extrema'):
        assert hasattr(SlabProblem, name)
    # the strides and sections of set_domain_series are checked on the host, with the same validator as the YAML key
    from gapflow_amd.series import _domain_series_entry
    assert _domain_series_entry({'integrals': np.int64(2)}, 13, 9) == {'integrals': 2, 'extrema': 0, 'sections_x': None, 'sections_y': None}
    with pytest.raises(ValueError, match=r'sections_x\[1\] = 14 lies outside the interior 1\.\.13'):
        _domain_series_entry({'integrals': 1, 'sections_x': [1, 14]}, 13, 9)
