"""fp64 NumPy restatement of the per-joint heat-map posterior under a Gaussian prior (metro_plan_bind_prior, include/metro_hip.h),
written unlike the kernel: dense arrays over the whole grid, the energy as one einsum of the offsets with the 3 x 3 precision
matrix, the moments as einsums of the probabilities with the grid -- no passes, no strides, no teams.  Also what the tests share:
the deviation measures and the recorded tolerances (profiles/heat_posterior_parity.json)."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = os.path.join(ROOT, 'profiles', 'heat_posterior_parity.json')
STATS = 11                      # log_evidence, peak', coords01' (x, y, z), cov01' (xx, yy, zz, xy, xz, yz)
PRIOR = 9                       # mu (x, y, z), precision (xx, yy, zz, xy, xz, yz)
COV6 = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
MEASURES = ('logev', 'peak', 'grid', 'cov')


def lin01(k):
    """tf.linspace(0, 1, k) as the soft-argmax evaluates it (fp32 step, fp32 product), as float64; one point: 0."""
    if k == 1:
        return np.zeros(1)
    return (np.arange(k, dtype=np.float32) * (np.float32(1.0) / np.float32(k - 1))).astype(np.float64)


def grid(side, depth):
    """[S(y), S(x), D, 3]: g(v) = (gx[x], gy[y], gz[d])."""
    gs, gd = lin01(side), lin01(depth)
    return np.stack(np.broadcast_arrays(gs[None, :, None], gs[:, None, None], gd[None, None, :]), -1)


def precision_matrix(words):
    """[..., 6] (xx, yy, zz, xy, xz, yz) -> [..., 3, 3]."""
    words = np.asarray(words, np.float64)
    lam = np.empty(words.shape[:-1] + (3, 3))
    for i, (a, b) in enumerate(COV6):
        lam[..., a, b] = lam[..., b, a] = words[..., i]
    return lam


def prior_rows(mu, lam):
    """mu [..., 3] and symmetric lam [..., 3, 3] -> the prior rows [..., 9] (fp64)."""
    lam = np.asarray(lam, np.float64)
    return np.concatenate([np.asarray(mu, np.float64), np.stack([lam[..., a, b] for a, b in COV6], -1)], -1)


def posterior(logits_nhwc, n_joints, depth, permutation, prior):
    """logits [N, S, S, D*J] (channel d*J + j) and prior [N, Jout, 9] -> post fp64 [N, Jout, 11], output joint order."""
    lg = np.asarray(logits_nhwc, np.float64)
    prior = np.asarray(prior, np.float64)
    n, s = lg.shape[0], lg.shape[1]
    perm = list(permutation)
    assert lg.shape == (n, s, s, depth * n_joints) and prior.shape == (n, len(perm), PRIOR), (lg.shape, prior.shape)
    g = grid(s, depth)
    post = np.full((n, len(perm), STATS), np.nan)
    with np.errstate(invalid='ignore', over='ignore', under='ignore', divide='ignore'):
        for i in range(n):
            vol = np.moveaxis(lg[i].reshape(s, s, depth, n_joints)[..., perm], -1, 0)             # [R, Y, X, D]
            off = g[None] - prior[i, :, None, None, None, :3]                                      # [R, Y, X, D, 3]
            q = -0.5 * np.einsum('ryxda,rab,ryxdb->ryxd', off, precision_matrix(prior[i, :, 3:]), off)
            w = vol + q
            m, mp = vol.max(axis=(1, 2, 3)), w.max(axis=(1, 2, 3))
            e, ep = np.exp(vol - m[:, None, None, None]), np.exp(w - mp[:, None, None, None])
            z, zp = e.sum(axis=(1, 2, 3)), ep.sum(axis=(1, 2, 3))
            p = ep / zp[:, None, None, None]
            mean = np.einsum('ryxd,yxdc->rc', p, g)
            dc = g[None] - mean[:, None, None, None, :]
            cov = np.einsum('ryxd,ryxda,ryxdb->rab', p, dc, dc)
            post[i, :, 0] = (mp - m) + np.log(zp / z)
            post[i, :, 1] = p.max(axis=(1, 2, 3))
            post[i, :, 2:5] = mean
            post[i, :, 5:] = np.stack([cov[:, a, b] for a, b in COV6], -1)
            bad = (np.isnan(prior[i]).any(-1) | np.isnan(vol).any(axis=(1, 2, 3)) | np.isposinf(vol).any(axis=(1, 2, 3)) |
                   ~np.isfinite(mp))
            post[i, bad] = np.nan
    return post


def deviation(got, ref, side, depth):
    """{'logev', 'peak', 'grid', 'cov'}: the largest |got - ref| of log_evidence (absolute), of peak' (in probability), of coords01'
    in grid steps (voxels), of cov01' in units of one voxel's variance (per element: the product of the two axes' grid steps),
    over the joints that are not NaN in the restatement."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    on = ~np.isnan(ref).any(-1)
    steps = np.array([max(side - 1, 1), max(side - 1, 1), max(depth - 1, 1)], np.float64)
    cov_scale = np.array([steps[a] * steps[b] for a, b in COV6])
    err = np.abs(got - ref)[on]
    worst = lambda e: float(e.max()) if e.size else 0.0
    return {'logev': worst(err[:, 0]), 'peak': worst(err[:, 1]), 'grid': worst(err[:, 2:5] * steps), 'cov': worst(err[:, 5:] * cov_scale)}


def recorded():
    """profiles/heat_posterior_parity.json: {'worst': {key: {'logev': .., 'peak': .., 'grid': .., 'cov': ..}}, ...}"""
    with open(PARITY) as f:
        return json.load(f)


GATE = 4.0              # the tests assert GATE x the recorded worst deviation of their key
EXACT = 1e-12           # the bound of the fp64 instantiations compiled for the host, in every measure


def gate(key):
    """Bounds of one recorded key.  They must stay far below what a wrong voxel costs: a tenth of a grid step in coords01'."""
    w = recorded()['worst'][key]
    g = {m: GATE * w[m] for m in MEASURES}
    assert g['grid'] < 0.1 and g['peak'] < 0.01, (key, g)
    return g


def check(got, ref, side, depth, bound, key, what=''):
    """The NaN joints exactly (all 11 values); prints the figures of the rest, then holds them to `bound` ({measure: value})."""
    got, ref = np.asarray(got), np.asarray(ref, np.float64)
    off = np.isnan(ref).any(-1)
    assert np.isnan(got[off]).all(), (key, what, 'poisoned joints')
    assert np.isfinite(got[~off]).all(), (key, what, 'finite joints')
    dev = deviation(got, ref, side, depth)
    print(f'heat_posterior {key} {what}: ' + ' '.join(f'{m} {dev[m]:.3e} (gate {bound[m]:.3e})' for m in MEASURES))
    assert all(dev[m] <= bound[m] for m in MEASURES), (key, what, dev, bound)
    return dev
