"""The cases of tests/golden/leaf_profiles.npz (outputs of the reference's models/profiles.py), rebuilt from the inputs
stored beside them: the CPU host check and the GPU tests of the profile operators read the fixture through this."""
import importlib.util
import os

import numpy as np

from helpers import GOLDEN

_spec = importlib.util.spec_from_file_location('make_profile_golden', os.path.join(GOLDEN, 'make_profile_golden.py'))
MAKER = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MAKER)
LEAF = np.load(os.path.join(GOLDEN, 'leaf_profiles.npz'))
INPUT_KEYS = ('q', 'h', 'dqx', 'dqy', 'Ls_field', 'z_shared', 'z_cell', 'point_q', 'point_h', 'point_dqx', 'point_dqy',
              'point_z', 'params')


def cases():
    """[(key, kind, kwargs, expected)]: kind 'velocity' or 'stress', expected (2 | 6, *result shape)."""
    d = {k: LEAF[k] for k in INPUT_KEYS}
    return [(key, kind, kw, LEAF[key]) for key, kind, kw in MAKER.cases(d)]


def scale_close(got, ref, tol):
    """max |got - ref| <= tol * max |ref|, per output."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-300)
    assert err <= tol, f'{err:.2e} of scale'
