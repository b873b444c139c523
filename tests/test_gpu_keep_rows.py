"""The keep-set of k_step2 changes where bytes live, never what they are: at the benchmark's size (4096^2 journal bearing, x-only gap,
DH), a handle that keeps k/8 of each step's rows in the Infinity Cache and one that streams every row with `nt` compute the same
bits.  The plan of a tuned handle names its keep choice."""
import contextlib
import os

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def environ(**env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run(steps, **env):
    """A headline problem, planned under `env` (read when the handle plans its first step), after `steps` steps."""
    from gapflow_amd import Problem
    with environ(**env):
        prob = Problem.from_string(bench.WORKLOAD_YAML.format(N=4096))
        prob._pre_run()
        prob._advance(steps, honor_stop=False)
    return prob


def scalars(prob):
    sc = prob._scalars()
    return {f[0]: getattr(sc, f[0]) for f in sc._fields_}


def test_keep_rows_do_not_change_the_result(hiplib):
    pinned = dict(GPF_CHUNKS=62, GPF_NT=2)
    a = run(20, GPF_KEEP_ROWS=0, **pinned)
    note_a = a._lib.gpf_plan_note(a._h).decode()
    qa, sa = a.q.copy(), scalars(a)
    del a
    b = run(20, GPF_KEEP_ROWS=4, **pinned)
    note_b = b._lib.gpf_plan_note(b._h).decode()
    assert 'keep 0/8 rows' in note_a and 'keep 4/8 rows' in note_b, (note_a, note_b)
    assert b.step == 20
    assert qa.tobytes() == b.q.tobytes()
    sb = scalars(b)
    for name in sa:
        assert np.asarray(sa[name]).tobytes() == np.asarray(sb[name]).tobytes(), (name, sa[name], sb[name])


def test_tuned_plan_names_the_keep_choice(hiplib):
    prob = run(3)
    note = prob._lib.gpf_plan_note(prob._h).decode()
    assert 'timed' in note, note
    if 'non-temporal' in note:
        assert 'rows on-die (timed, us: k 0 ' in note, note
    assert prob._scalars().invalid == 0
