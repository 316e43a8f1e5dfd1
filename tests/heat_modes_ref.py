"""fp64 NumPy restatement of the per-joint heat-map modes (metro_plan_bind_modes, include/metro_hip.h), written unlike the
kernel: candidates from 26 shifted comparisons on a -inf padded array, selection as a Python `sorted` over all candidates plus
a distance check against a list, windows as slices with np.average / np.cov -- no slabs, no flags, no rounds, no ladders.
Also what the tests share: the deviation measures and the recorded tolerances (profiles/heat_modes_parity.json)."""
import itertools
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = os.path.join(ROOT, 'profiles', 'heat_modes_parity.json')
STATS = 11                      # mass, peak, coords01 (x, y, z), cov01 (xx, yy, zz, xy, xz, yz)
COV6 = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
SMALL_MASS = 1e-6               # below it (in the restatement) a mode is compared in voxel and mass only


def lin01(k):
    """tf.linspace(0, 1, k) as the soft-argmax evaluates it (fp32 step, fp32 product), as float64; one point: 0."""
    if k == 1:
        return np.zeros(1)
    return (np.arange(k, dtype=np.float32) * (np.float32(1.0) / np.float32(k - 1))).astype(np.float64)


def candidates(vol):
    """bool [S, S, D]: finite voxels that beat all their neighbours (an equal one only if it comes later in linear order)."""
    s, _, d = vol.shape
    pad = np.full((s + 2, s + 2, d + 2), -np.inf)
    pad[1:-1, 1:-1, 1:-1] = vol
    ok = np.isfinite(vol)
    for shift in itertools.product((-1, 0, 1), repeat=3):
        if shift == (0, 0, 0):
            continue
        nb = pad[1 + shift[0]:1 + shift[0] + s, 1 + shift[1]:1 + shift[1] + s, 1 + shift[2]:1 + shift[2] + d]
        ok &= (nb < vol) | ((nb == vol) & (shift > (0, 0, 0)))
    return ok


def select(vol, k, radius):
    """The (y, x, d) of at most k modes: candidates by decreasing logit, ties by increasing index, none within 2 radius of another."""
    s, _, d = vol.shape
    cands = sorted((tuple(c) for c in np.argwhere(candidates(vol))), key=lambda c: (-vol[c], (c[0] * s + c[1]) * d + c[2]))
    chosen = []
    for c in cands:
        if len(chosen) == k:
            break
        if all(max(abs(a - b) for a, b in zip(c, m)) > 2 * radius for m in chosen):
            chosen.append(c)
    return chosen


def joint_modes(vol, k, radius):
    """One joint's volume [S, S, D] (fp64) -> (voxel [k], stats [k, 11])."""
    s, _, d = vol.shape
    voxel, stats = np.full(k, -1, np.int32), np.full((k, STATS), np.nan)
    if np.isnan(vol).any() or np.isposinf(vol).any():
        return voxel, stats
    stats[:, 0] = 0.0
    chosen = select(vol, k, radius)
    if not chosen:
        return voxel, stats
    m = vol.max()
    with np.errstate(under='ignore'):
        p = np.exp(vol - (m + np.log(np.exp(vol - m).sum())))
    gs, gd = lin01(s), lin01(d)
    for i, (y, x, z) in enumerate(chosen):
        ys, xs, zs = (slice(max(c - radius, 0), c + radius + 1) for c in (y, x, z))
        w = p[ys, xs, zs].reshape(-1)
        pts = np.stack([g.reshape(-1) for g in np.broadcast_arrays(gs[None, xs, None], gs[ys, None, None], gd[None, None, zs])])
        voxel[i] = (y * s + x) * d + z
        stats[i, 0], stats[i, 1] = w.sum(), p[y, x, z]
        stats[i, 2:5] = np.average(pts, axis=1, weights=w)
        cov = np.atleast_2d(np.cov(pts, aweights=w, bias=True))
        stats[i, 5:] = [cov[a, b] for a, b in COV6]
    return voxel, stats


def modes(logits_nhwc, n_joints, depth, permutation, k, radius):
    """logits [N, S, S, D*J] (channel d*J + j) -> (voxel int32 [N, Jout, k], stats fp64 [N, Jout, k, 11]), output joint order."""
    lg = np.asarray(logits_nhwc, np.float64)
    n, s = lg.shape[0], lg.shape[1]
    assert lg.shape == (n, s, s, depth * n_joints), lg.shape
    voxel, stats = np.empty((n, len(permutation), k), np.int32), np.empty((n, len(permutation), k, STATS))
    for i in range(n):
        vol = lg[i].reshape(s, s, depth, n_joints)
        done = {}
        for r, j in enumerate(permutation):
            if j not in done:
                done[j] = joint_modes(vol[..., j], k, radius)
            voxel[i, r], stats[i, r] = done[j]
    return voxel, stats


def deviation(got, ref_voxel, ref_stats, side, depth):
    """{'prob', 'grid', 'cov'}: the largest |got - ref| of mass and peak in probability, of coords01 in grid units (voxels), of
    cov01 relative to one voxel's variance (per element: the product of the two axes' grid steps).  Emitted modes only; a mode
    whose mass in the restatement is below SMALL_MASS enters with its mass only."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref_stats, np.float64)
    on = np.asarray(ref_voxel) >= 0
    full = on & (ref[..., 0] >= SMALL_MASS)
    steps = np.array([max(side - 1, 1), max(side - 1, 1), max(depth - 1, 1)], np.float64)
    cov_scale = np.array([steps[a] * steps[b] for a, b in COV6])
    err = np.abs(got - ref)
    worst = lambda e: float(e.max()) if e.size else 0.0
    return {'prob': max(worst(err[on][:, 0]), worst(err[full][:, 1])), 'grid': worst(err[full][:, 2:5] * steps),
            'cov': worst(err[full][:, 5:] * cov_scale)}


def small_fraction(ref_voxel, ref_stats):
    """The share of the emitted modes whose mass is below SMALL_MASS."""
    on = np.asarray(ref_voxel) >= 0
    return float((np.asarray(ref_stats)[..., 0][on] < SMALL_MASS).mean()) if on.any() else 0.0


def recorded():
    """profiles/heat_modes_parity.json: {'worst': {key: {'prob': .., 'grid': .., 'cov': ..}}, ...}"""
    with open(PARITY) as f:
        return json.load(f)


GATE = 4.0              # the tests assert GATE x the recorded worst deviation of their key


def gate(key):
    """Bounds of one recorded key.  They must stay far below what a wrong voxel costs: a tenth of a grid step in coords01."""
    w = recorded()['worst'][key]
    g = {m: GATE * w[m] for m in ('prob', 'grid', 'cov')}
    assert g['grid'] < 0.1 and g['prob'] < 0.01, (key, g)
    return g


def check(got_voxel, got_stats, ref_voxel, ref_stats, side, depth, key, what=''):
    """voxel exactly; the missing and poisoned modes exactly (mass 0 or NaN, NaN elsewhere); prints the figures of the rest,
    then holds them to the gate of `key`."""
    got_voxel, got_stats = np.asarray(got_voxel), np.asarray(got_stats)
    assert np.array_equal(got_voxel, ref_voxel), (key, what, 'voxel', int((got_voxel != ref_voxel).sum()))
    off = np.asarray(ref_voxel) < 0
    assert np.array_equal(got_stats[off], np.asarray(ref_stats, np.float32)[off], equal_nan=True), (key, what, 'missing modes')
    assert np.isfinite(got_stats[~off][:, 0]).all(), (key, what)
    dev, bound = deviation(got_stats, ref_voxel, ref_stats, side, depth), gate(key)
    print(f'heat_modes {key} {what}: ' + ' '.join(f'{m} {dev[m]:.3e} (gate {bound[m]:.3e})' for m in ('prob', 'grid', 'cov')))
    assert all(dev[m] <= bound[m] for m in dev), (key, what, dev, bound)
