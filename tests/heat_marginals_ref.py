"""fp64 NumPy restatement of the per-joint heat-map marginals (metro_plan_bind_heatmaps), written unlike the kernels: per
(crop, output joint) one [S, S, D] view of the logits, a log-sum-exp over the whole view, then np.sum over axes -- no tiles, no
per-channel records, no folds.  Also what the tests share: the cases, the deviation measure and the recorded tolerances."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = os.path.join(ROOT, 'profiles', 'heat_marginals_parity.json')


def lin01(k):
    """tf.linspace(0, 1, k) as the soft-argmax evaluates it (fp32 step, fp32 product), as float64."""
    return (np.arange(k, dtype=np.float32) * (np.float32(1.0) / np.float32(k - 1))).astype(np.float64)


def logsumexp(v):
    """log sum exp of all of v; NaN when v holds a NaN or +Inf (no distribution), -Inf entries are weight zero."""
    v = np.asarray(v, np.float64)
    if np.isnan(v).any() or np.isposinf(v).any():
        return np.nan
    m = v.max()
    if np.isneginf(m):
        return np.nan
    with np.errstate(under='ignore'):
        return m + np.log(np.exp(v - m).sum())


def marginals(logits_nhwc, n_joints, depth, permutation):
    """logits [N, S, S, D*J] (channel d*J + j) -> (xy [N, Jout, S, S], z [N, Jout, D]) in fp64, output joint order."""
    lg = np.asarray(logits_nhwc, np.float64)
    n, s = lg.shape[0], lg.shape[1]
    assert lg.shape == (n, s, s, depth * n_joints), lg.shape
    xy = np.empty((n, len(permutation), s, s))
    z = np.empty((n, len(permutation), depth))
    for i in range(n):
        vol = lg[i].reshape(s, s, depth, n_joints)
        for r, j in enumerate(permutation):
            v = vol[..., j]
            with np.errstate(invalid='ignore', under='ignore'):
                p = np.exp(v - logsumexp(v))
            xy[i, r] = np.sum(p, axis=2)
            z[i, r] = np.sum(p, axis=(0, 1))
    return xy, z


def expectations(xy, z):
    """coords01 [N, Jout, 3] of the marginals on the soft-argmax grids."""
    xy, z = np.asarray(xy, np.float64), np.asarray(z, np.float64)
    gs, gd = lin01(xy.shape[-1]), lin01(z.shape[-1])
    return np.stack([(xy.sum(axis=2) * gs).sum(-1), (xy.sum(axis=3) * gs).sum(-1), (z * gd).sum(-1)], axis=-1)


def deviation(got, ref):
    """(largest |got - ref| in probability, largest |got - ref| relative to its row's largest reference entry); a row is one
    joint's map ([S, S] flattened, or [D])."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.ndim == 4:
        got, ref = got.reshape(*got.shape[:2], -1), ref.reshape(*ref.shape[:2], -1)
    err = np.abs(got - ref)
    return float(err.max()), float((err.max(-1) / ref.max(-1)).max())


def recorded():
    """profiles/heat_marginals_parity.json: {'worst': {key: {'abs': .., 'rel': ..}}, ...}"""
    with open(PARITY) as f:
        return json.load(f)


GATE = 4.0              # the tests assert GATE x the recorded worst deviation of their key


def gate(key, smallest_voxels):
    """(abs, rel) bounds of one recorded key.  The absolute bound must stay below 1 / (S*S*D) of the smallest head of the key --
    the probability of one voxel of a flat map -- so that a misplaced voxel can never pass."""
    w = recorded()['worst'][key]
    a, r = GATE * w['abs'], GATE * w['rel']
    assert a < 1.0 / smallest_voxels, (key, a, smallest_voxels)
    return a, r


def check(got_xy, got_z, ref_xy, ref_z, key, smallest_voxels, what=''):
    """Prints the figures, then holds them to the gate of `key`."""
    bound_a, bound_r = gate(key, smallest_voxels)
    for name, got, ref in (('xy', got_xy, ref_xy), ('z', got_z, ref_z)):
        a, r = deviation(got, ref)
        print(f'heat_marginals {key} {what} {name}: abs {a:.3e} (gate {bound_a:.3e}) rel {r:.3e} (gate {bound_r:.3e})')
        assert a <= bound_a and r <= bound_r, (key, what, name, a, bound_a, r, bound_r)
