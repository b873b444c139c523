"""Cost of point probes: what they cost when off, and what a record per step costs when on.

    python tools/probe_time.py [--n 4096] [--steps 200] [--small-steps 4000] [--rounds 7] [--parent PATH.so] [--json FILE]

One process, alternating legs, one warm-up round that is thrown away, then --rounds rounds; every figure is printed with its
median and its whole range.
  * 4096^2 journal bearing (bench.py's workload, k_step2), gpf_probes_time over --steps steps, HIP events on the handle's stream:
    off      no probes                                      (the parent commit's launches)
    empty    an empty kernel behind every step              (the floor of "one more launch per step")
    probes   16 probes with pressure, k_probe_record behind every step
    added = leg - off per step, and the ratio added(probes) / added(empty).
  * Nx = 100 journal bearing (k_small_steps), gpf_step of --small-steps steps in one launch, wall clock: off, and 7 probes with
    pressure recorded inside the kernel.
  * --parent: the same two problems on the parent commit's library in the same process (its own handles), gpf_step wall clock
    for both libraries, legs alternating parent / this: is "probes off" inside the parent's own run-to-run range?"""
import argparse
import contextlib
import ctypes as C
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LARGE = """
options: {{silent: True}}
grid: {{dx: 1.e-5, dy: 1.e-5, Nx: {n}, Ny: {n}, xE: ['P', 'P', 'P'], xW: ['P', 'P', 'P'], yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P']}}
geometry: {{type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.}}
numerics: {{CFL: 0.5, adaptive: 1, tol: 1e-12, dt: 1e-10, max_it: 100000000}}
properties: {{shear: 0.0794, bulk: 0., EOS: DH, P0: 101325., rho0: 877.7007, C1: 3.5e10, C2: 1.23}}
"""
SMALL = """
options: {silent: True}
grid: {dx: 1.e-5, dy: 1., Nx: 100, Ny: 1, xE: ['D', 'N', 'N'], xW: ['D', 'N', 'N'], yS: ['P', 'P', 'P'], yN: ['P', 'P', 'P'],
       xE_D: 877.7007, xW_D: 877.7007}
geometry: {type: journal, CR: 1.e-2, eps: 0.7, U: 0.1, V: 0.}
numerics: {CFL: 0.25, adaptive: 1, tol: 1e-12, dt: 1e-10, max_it: 100000000}
properties: {shear: 0.0794, bulk: 0., EOS: DH, P0: 101325, rho0: 877.7007, C1: 3.5e10, C2: 1.23}
"""
CELLS_SMALL = [(0, 1), (1, 1), (50, 1), (100, 1), (101, 1), (50, 0), (50, 2)]


def stats(v):
    return {'median': statistics.median(v), 'min': min(v), 'max': max(v), 'all': list(v)}


def build(text, lib=None):
    """A problem after _pre_run and a few steps; `lib`: on that library instead of the package's."""
    from gapflow_amd import Problem, _lib
    saved = _lib._lib
    if lib is not None:
        _lib._lib = lib
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            p = Problem.from_string(text)
            p._pre_run()
            p._advance(4, honor_stop=False)
    finally:
        _lib._lib = saved
    return p


def load_parent(path):
    from gapflow_amd import _lib
    _lib.load()
    lib = C.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(lib, name):              # the parent has no gpf_probes_*
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def step_wall(p, n):
    """gpf_step of n steps (returns after a stream sync): wall seconds per step"""
    from gapflow_amd import _lib
    nexec = C.c_int64(0)
    t0 = time.perf_counter()
    rc = p._lib.gpf_step(p._h, n, 0, None, 0, C.byref(nexec))
    dt = time.perf_counter() - t0
    if rc != 0:
        raise _lib.GapflowHipError(p._lib.gpf_last_error().decode())
    return dt / n


def probes_time(p, n, mode):
    from gapflow_amd import _lib
    ms = C.c_double(0.)
    _lib.check(p._lib.gpf_probes_time(p._h, n, mode, C.byref(ms)))
    return ms.value / n


def main(argv=None):
    cli = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    cli.add_argument('--n', type=int, default=4096)
    cli.add_argument('--steps', type=int, default=200)
    cli.add_argument('--small-steps', type=int, default=4000)
    cli.add_argument('--rounds', type=int, default=7)
    cli.add_argument('--parent', metavar='PATH.so')
    cli.add_argument('--json', metavar='FILE')
    o = cli.parse_args(argv)
    out = {'n': o.n, 'steps': o.steps, 'small_steps': o.small_steps, 'rounds': o.rounds}

    # ---- probes on, 4096^2: against an empty launch in the same stream position ----
    big = build(LARGE.format(n=o.n))
    rows = [1 + (k * (o.n - 1)) // 15 for k in range(16)]
    big.set_probes([(r, 1 + (7 * r) % o.n) for r in rows], pressure=True)
    legs = {'off': 0, 'empty': 2, 'probes': 1}
    t = {k: [] for k in legs}
    for r in range(o.rounds + 1):
        for k, mode in legs.items():
            ms = probes_time(big, o.steps, mode)
            if r:
                t[k].append(ms)
    out['large_ms_per_step'] = {k: stats(v) for k, v in t.items()}
    add_e = [a - b for a, b in zip(t['empty'], t['off'])]
    add_p = [a - b for a, b in zip(t['probes'], t['off'])]
    out['large_added_us_per_step'] = {'empty': stats([1e3 * x for x in add_e]), 'probes': stats([1e3 * x for x in add_p])}
    out['large_added_ratio_of_medians'] = statistics.median(add_p) / statistics.median(add_e) if statistics.median(add_e) > 0 else None

    # ---- small grid: recording inside k_small_steps ----
    s_off, s_on = build(SMALL), build(SMALL)
    s_on.set_probes(CELLS_SMALL, pressure=True)
    t = {'off': [], 'probes': []}
    for r in range(o.rounds + 1):
        for k, p in (('off', s_off), ('probes', s_on)):
            us = 1e6 * step_wall(p, o.small_steps)
            if r:
                t[k].append(us)
    out['small_us_per_step'] = {k: stats(v) for k, v in t.items()}
    assert len(s_on.probes.step) == 0       # (gpf_step was called directly: the records stay in the library)

    # ---- probes off against the parent commit's library ----
    if o.parent:
        par = load_parent(o.parent)
        big.clear_probes()
        pairs = {'large_ms_per_step': (build(LARGE.format(n=o.n), par), big, o.steps, 1e3),
                 'small_us_per_step': (build(SMALL, par), s_off, o.small_steps, 1e6)}
        for key, (pp, pt, n, scale) in pairs.items():
            t = {'parent': [], 'this': []}
            for r in range(o.rounds + 1):
                for k, p in (('parent', pp), ('this', pt)):
                    v = scale * step_wall(p, n)
                    if r:
                        t[k].append(v)
            out['off_vs_parent_' + key] = {k: stats(v) for k, v in t.items()}
            a, b = out['off_vs_parent_' + key]['parent'], out['off_vs_parent_' + key]['this']
            out['off_vs_parent_' + key]['this_median_inside_parent_range'] = a['min'] <= b['median'] <= a['max']

    def line(name, s, unit):
        print(f"{name:34s} median {s['median']:.4f} {unit}   range {s['min']:.4f} .. {s['max']:.4f}")
    for k, s in out['large_ms_per_step'].items():
        line(f"{o.n}^2 {k}", s, 'ms/step')
    for k, s in out['large_added_us_per_step'].items():
        line(f"{o.n}^2 added by {k}", s, 'us/step')
    print(f"added(probes) / added(empty), medians: {out['large_added_ratio_of_medians']}")
    for k, s in out['small_us_per_step'].items():
        line(f"Nx=100 {k}", s, 'us/step')
    for key in ('large_ms_per_step', 'small_us_per_step'):
        d = out.get('off_vs_parent_' + key)
        if d:
            for k in ('parent', 'this'):
                line(f"probes off, {key.split('_')[0]}, {k}", d[k], key.split('_')[1] + '/step')
            print(f"  this library's median inside the parent's range: {d['this_median_inside_parent_range']}")
    if o.json:
        os.makedirs(os.path.dirname(os.path.abspath(o.json)), exist_ok=True)
        with open(o.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
