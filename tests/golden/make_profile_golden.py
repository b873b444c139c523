"""Regenerates leaf_profiles.npz: true outputs of the reference's GaPFlow/models/profiles.py (get_velocity_profiles,
get_stress_profiles) on seeded inputs.

    python tests/golden/make_profile_golden.py [REFERENCE_ROOT]

profiles.py imports nothing, so it is loaded by path from the reference checkout (default: the environment variable
GAPFLOW_REFERENCE, else ../reference beside this repository).  Before anything is written, the slip-parabola restatement
that csrc/closures.hpp evaluates (profile_coefficients / profile_at) is restated here in NumPy and checked against the
reference at 1e-13 of each output's scale.  The archive is written with fixed zip timestamps, so a second run reproduces
it bit for bit.

Cases: every mode (both, top, bottom, none) x gradients zero / nonzero x slip length scalar / per cell x z shared
(nz, 1, 1) / per cell (nz, nx, ny), on one small field with U and V nonzero; plus point inputs q (3,) with z (nz,).
"""
import importlib.util
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'leaf_profiles.npz')
MODES = ('both', 'top', 'bottom', 'none')
SEED = 20261016
NX, NY, NZ = 3, 4, 6
U, V, ETA, ZETA, LS = 0.7, -0.4, 0.9, 0.3, 0.35


def load_reference(root):
    path = os.path.join(root, 'GaPFlow', 'models', 'profiles.py')
    spec = importlib.util.spec_from_file_location('ref_profiles', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def inputs():
    rng = np.random.default_rng(SEED)
    d = {}
    d['q'] = np.stack([rng.uniform(0.8, 1.2, (NX, NY)), rng.uniform(-0.5, 1.5, (NX, NY)), rng.uniform(-0.8, 0.8, (NX, NY))])
    d['h'] = np.stack([rng.uniform(0.5, 1.5, (NX, NY)), rng.uniform(-0.1, 0.1, (NX, NY)), rng.uniform(-0.1, 0.1, (NX, NY))])
    d['dqx'] = rng.uniform(-0.3, 0.3, (3, NX, NY))
    d['dqy'] = rng.uniform(-0.3, 0.3, (3, NX, NY))
    d['Ls_field'] = rng.uniform(0.0, 0.6, (NX, NY))
    d['z_shared'] = np.linspace(0.0, 1.1, NZ)[:, None, None]
    d['z_cell'] = d['h'][0][None] * np.linspace(0.0, 1.0, NZ)[:, None, None]
    d['point_q'] = np.array([1.05, 0.8, -0.3])
    d['point_h'] = np.array([1.2, 0.03, -0.02])
    d['point_dqx'] = np.array([0.1, -0.2, 0.05])
    d['point_dqy'] = np.array([-0.07, 0.12, 0.2])
    d['point_z'] = np.linspace(0.0, 1.2, 9)
    d['params'] = np.array([U, V, ETA, ZETA, LS])
    return d


# ---- the restatement evaluated by csrc/closures.hpp ----------------------------------------------------------------
def slip(mode, Ls):
    lo = Ls if mode in ('both', 'bottom') else 0.0 * Ls
    hi = Ls if mode in ('both', 'top') else 0.0 * Ls
    return lo, hi


def parabola(h, W, m, lo, hi):
    D = h * h + 4 * h * (lo + hi) + 12 * lo * hi
    Dh = 2 * h + 4 * (lo + hi)
    Na = 3 * (h + 2 * hi) * W - 6 * (h + lo + hi) * m
    Nb = -4 * (h + 3 * hi) * W + 6 * (h + 2 * hi) * m
    Nc = h * (h + 4 * hi) * W + 6 * lo * (h + 2 * hi) * m
    a, b, c = Na / (h * D), Nb / D, Nc / D
    ah = ((3 * W - 6 * m) * (h * D) - Na * (D + h * Dh)) / (h * D) ** 2
    bh = ((-4 * W + 6 * m) * D - Nb * Dh) / D ** 2
    ch = (((2 * h + 4 * hi) * W + 6 * lo * m) * D - Nc * Dh) / D ** 2
    am, bm, cm = -6 * (h + lo + hi) / (h * D), 6 * (h + 2 * hi) / D, 6 * lo * (h + 2 * hi) / D
    return a, b, c, ah, bh, ch, am, bm, cm


def restated_velocity(z, q, Ls, U, V, mode):
    h = z[-1]
    lo, hi = slip(mode, Ls)
    out = []
    for W, j in ((U, q[1]), (V, q[2])):
        a, b, c = parabola(h, W, j / q[0], lo, hi)[:3]
        out.append((a * z + b) * z + c)
    return out


def restated_stress(z, h, q, dqx, dqy, U, V, eta, zeta, Ls, mode):
    lo, hi = slip(mode, Ls)
    mu, mv = q[1] / q[0], q[2] / q[0]
    pu, pv = parabola(h[0], U, mu, lo, hi), parabola(h[0], V, mv, lo, hi)

    def d(p, hd, md):
        return [p[3 + k] * hd + p[6 + k] * md for k in range(3)]

    def at(c):
        return (c[0] * z + c[1]) * z + c[2]

    ux = at(d(pu, h[1], (dqx[1] - mu * dqx[0]) / q[0]))
    uy = at(d(pu, h[2], (dqy[1] - mu * dqy[0]) / q[0]))
    vx = at(d(pv, h[1], (dqx[2] - mv * dqx[0]) / q[0]))
    vy = at(d(pv, h[2], (dqy[2] - mv * dqy[0]) / q[0]))
    v1, v2 = zeta + 4 / 3 * eta, zeta - 2 / 3 * eta
    return (v1 * ux + v2 * vy, v2 * ux + v1 * vy, v2 * (ux + vy), eta * (2 * pv[0] * z + pv[1]),
            eta * (2 * pu[0] * z + pu[1]), eta * (uy + vx))


def cases(d):
    """(key, kind, kwargs) for every stored output."""
    U_, V_, eta, zeta, Ls = d['params']
    for mode in MODES:
        for grad in (0, 1):
            for zf in ('shared', 'cell'):
                for lsf in ('scalar', 'field'):
                    Lsv = Ls if lsf == 'scalar' else d['Ls_field']
                    z = d['z_' + zf]
                    dqx = d['dqx'] * grad
                    dqy = d['dqy'] * grad
                    yield (f'stress_{mode}_g{grad}_{zf}_{lsf}', 'stress',
                           dict(z=z, h=d['h'], q=d['q'], dqx=dqx, dqy=dqy, U=U_, V=V_, eta=eta, zeta=zeta, Ls=Lsv, mode=mode))
                    if grad == 0:
                        yield (f'velocity_{mode}_{zf}_{lsf}', 'velocity', dict(z=z, q=d['q'], Ls=Lsv, U=U_, V=V_, slip=mode))
        for grad in (0, 1):
            yield (f'point_stress_{mode}_g{grad}', 'stress',
                   dict(z=d['point_z'], h=d['point_h'], q=d['point_q'], dqx=d['point_dqx'] * grad, dqy=d['point_dqy'] * grad,
                        U=U_, V=V_, eta=eta, zeta=zeta, Ls=Ls, mode=mode))
        yield (f'point_velocity_{mode}', 'velocity', dict(z=d['point_z'], q=d['point_q'], Ls=Ls, U=U_, V=V_, slip=mode))


def scale_err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def write_npz(path, arrays):
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, 'w', compression=zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            with zf.open(info, 'w', force_zip64=True) as f:
                np.lib.format.write_array(f, np.ascontiguousarray(arrays[key]), allow_pickle=False)
    with open(path, 'wb') as f:
        f.write(buf.getvalue())


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get(
        'GAPFLOW_REFERENCE', os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(HERE))), 'reference'))
    ref = load_reference(root)
    d = inputs()
    out = dict(d)
    worst = 0.0
    for key, kind, kw in cases(d):
        if kind == 'stress':
            got = np.array(np.broadcast_arrays(*ref.get_stress_profiles(**kw)))
            mine = restated_stress(kw['z'], kw['h'], kw['q'], kw['dqx'], kw['dqy'], kw['U'], kw['V'], kw['eta'], kw['zeta'],
                                   kw['Ls'], kw['mode'])
        else:
            got = np.array(np.broadcast_arrays(*ref.get_velocity_profiles(**kw)))
            mine = restated_velocity(kw['z'], kw['q'], kw['Ls'], kw['U'], kw['V'], kw['slip'])
        for c in range(len(got)):
            e = scale_err(np.broadcast_to(mine[c], got[c].shape), got[c])
            worst = max(worst, e)
            assert e <= 1e-13, (key, c, e)
        out[key] = got
    write_npz(OUT, out)
    print(f'restatement vs reference: worst {worst:.2e} of scale; wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(out)} arrays)')


if __name__ == '__main__':
    main()
