"""Row f4: evaluation metrics (MPJPE, Procrustes-MPJPE, PCK, AUC) -- oracle known answers on CPU,
HIP kernels vs oracle on the GPU."""
import numpy as np
import pytest

from oracle.metrics import eval_metrics as oracle_metrics


def _poses(n=50, nj=17, seed=0):
    rng = np.random.default_rng(seed)
    true = (rng.standard_normal((n, nj, 3)) * 250).astype(np.float32)
    pred = true + (rng.standard_normal((n, nj, 3)) * 60).astype(np.float32)
    valid = rng.random((n, nj)) > 0.15
    valid[:, :4] = True
    return pred, true, valid


def _rot(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q * np.sign(np.linalg.det(q))


def test_rigid_motion_and_scale_are_removed_by_alignment():
    rng = np.random.default_rng(1)
    _, true, _ = _poses(8)
    pred = np.stack([(1.7 * t @ _rot(rng) + rng.standard_normal(3) * 300) for t in true]).astype(np.float32)
    m = oracle_metrics(pred, true)
    assert m['mean_error'] > 50 and m['mean_error_procrustes'] < 1e-3


def test_reflection_is_not_allowed():
    _, true, _ = _poses(4, seed=2)
    pred = true * np.array([-1, 1, 1], np.float32)             # mirrored pose
    m = oracle_metrics(pred, true)
    assert m['mean_error_procrustes'] > 10                      # a reflection would give 0


def test_plain_metrics_known_values():
    true = (np.random.default_rng(0).standard_normal((2, 3, 3)) * 100).astype(np.float32)
    pred = true.copy()
    pred[0, 0] += [30, 40, 0]         # 50 mm
    pred[1, 1] += [0, 0, 300]         # 300 mm
    m = oracle_metrics(pred, true, np.ones((2, 3), bool))
    assert np.isclose(m['mean_error'], (50 + 300) / 6)
    assert np.allclose(m['pck'], [1, 0.5, 1]) and np.isclose(m['mean_pck'], 5 / 6)
    assert np.allclose(m['auc'], [(1 - 50 / 150 + 1) / 2, 0.5, 1])
    # root-relative: moving the root (last joint) moves every other joint's error
    pred2 = pred.copy()
    pred2[:, 2] += [0, 10, 0]
    d2 = oracle_metrics(pred2, true)['dist']
    assert np.isclose(d2[0, 2], 0) and np.isclose(d2[1, 0], 10, atol=1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize('masked', [False, True])
def test_hip_metrics_match_oracle(cuda, masked):
    import torch
    from metro_pose3d_amd.metrics import eval_metrics
    pred, true, valid = _poses(300, 19, seed=3)
    rng = np.random.default_rng(4)
    pred[:20] = np.stack([(1.3 * t @ _rot(rng) + 100) for t in true[:20]])       # exact similarity transforms
    pred[20:30] = true[20:30] * np.array([-1, 1, 1], np.float32)                 # reflections
    v = valid if masked else None
    ref = oracle_metrics(pred, true, v)
    got = eval_metrics(torch.from_numpy(pred).to(cuda), torch.from_numpy(true).to(cuda),
                       torch.from_numpy(valid).to(cuda) if masked else None)
    assert np.abs(got['dist'].cpu().numpy() - ref['dist']).max() < 1e-3
    assert np.abs(got['dist_procrustes'].cpu().numpy() - ref['dist_procrustes']).max() < 2e-3, \
        np.abs(got['dist_procrustes'].cpu().numpy() - ref['dist_procrustes']).max()
    for k in ('mean_error', 'mean_error_procrustes', 'mean_auc', 'mean_pck'):
        assert abs(got[k] - ref[k]) < 1e-4 * max(1.0, abs(ref[k])), k
    assert np.allclose(got['auc'], ref['auc'], atol=1e-5) and np.allclose(got['pck'], ref['pck'], atol=1e-6)


# ---- the kernels on degenerate poses, ragged n and masks ------------------------------------------------------------------

FAMILIES = ('generic', 'both planar', 'truth planar', 'near-planar', 'near-collinear', 'exact mirror', 'absolute',
            'pred == truth', 'similarity')


def _family_poses(n, nj, seed):
    """n pose pairs, pose i of family (i + seed) % 9, root joint last.  -> (pred, true, family index [n])."""
    rng = np.random.default_rng([n, nj, seed])
    true = rng.standard_normal((n, nj, 3)) * 250
    pred = true + rng.standard_normal((n, nj, 3)) * 60
    fam = (np.arange(n) + seed) % len(FAMILIES)
    for i, f in enumerate(fam):
        name = FAMILIES[f]
        if name == 'both planar':
            true[i, :, 2] = 0; pred[i, :, 2] = 0
        elif name == 'truth planar':
            true[i, :, 2] = 0
        elif name == 'near-planar':
            true[i, :, 2] *= 1e-5; pred[i, :, 2] *= 1e-5
        elif name == 'near-collinear':
            true[i, :, 1:] *= 1e-4; pred[i, :, 1:] *= 1e-4
        elif name == 'exact mirror':
            pred[i] = true[i] * [-1, 1, 1]
        elif name == 'absolute':
            off = rng.uniform(-5000, 5000, 3)
            true[i] += off; pred[i] += off + rng.standard_normal(3) * 40
        elif name == 'pred == truth':
            pred[i] = true[i]
        elif name == 'similarity':
            pred[i] = 1.3 * true[i] @ _rot(rng) + rng.standard_normal(3) * 300
    return pred.astype(np.float32), true.astype(np.float32), fam


def _gpu_metrics(cuda, pred, true, valid):
    import torch
    from metro_pose3d_amd.metrics import eval_metrics
    got = eval_metrics(torch.from_numpy(pred).to(cuda), torch.from_numpy(true).to(cuda),
                       torch.from_numpy(valid).to(cuda) if valid is not None else None)
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in got.items()}


@pytest.mark.gpu
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('nj', [3, 17, 53])
def test_hip_metrics_on_degenerate_poses_and_ragged_batches(cuda, nj, masked):
    """eval_pose_kernel / eval_reduce_kernel against oracle/metrics.py (LAPACK SVD) where a Jacobi-on-A^T A Procrustes and a
    strided block reduction go wrong if they are wrong: planar, near-planar (z x 1e-5) and near-collinear (y, z x 1e-4) poses,
    an exact mirror image, poses in absolute coordinates +-5 m, pred == truth and exact similarities, interleaved pose by
    pose, at 3 / 17 / 53 joints and n = 1, 63, 64, 65, 257 and 5000 (a 64-lane block more or less; 20 strides of the
    reduction's 256 threads).  Masked: random masks that keep >= 3 joints (the alignment is defined), a joint column with no
    valid entry (its per-joint PCK / AUC NaN on both sides, the overall means untouched) and an invalid root joint in
    every third pose; at 3 joints the mask is all ones.  Bounds as in test_hip_metrics_match_oracle: 1e-3 mm on dist, 2e-3 mm
    on dist_procrustes, 1e-4 relative on the means, 1e-5 / 1e-6 on per-joint AUC / PCK.
    Measured on the MI355X: dist_procrustes at most 1.0e-4 mm from the oracle (absolute coordinates, 3 joints), 8.9e-5 mm
    at 17 / 53 joints (exact mirror), 6e-12 mm on exact similarities."""
    worst = np.zeros(len(FAMILIES))
    for n in (1, 63, 64, 65, 257, 5000):
        for seed in (range(len(FAMILIES)) if n == 1 else (n % len(FAMILIES),)):
            pred, true, fam = _family_poses(n, nj, seed)
            valid = None
            if masked:
                rng = np.random.default_rng([n, nj, seed, 1])
                valid = np.ones((n, nj), bool)
                if nj > 3:
                    valid = rng.random((n, nj)) > 0.3
                    valid[:, 2:5] = True
                    valid[:, 1] = False                                     # a joint nobody has
                    valid[::3, -1] = False                                  # an invalid root joint
            with np.errstate(invalid='ignore', divide='ignore'):
                ref = oracle_metrics(pred, true, valid)
            got = _gpu_metrics(cuda, pred, true, valid)
            assert np.isfinite(ref['dist_procrustes']).all() and np.isfinite(got['dist_procrustes']).all(), (n, seed)
            assert np.abs(got['dist'] - ref['dist']).max() < 1e-3, (n, seed)
            epa = np.abs(got['dist_procrustes'] - ref['dist_procrustes']).max(axis=1)
            np.maximum.at(worst, fam, epa)
            assert epa.max() < 2e-3, (n, seed, [(FAMILIES[f], e) for f, e in zip(fam, epa) if e >= 2e-3][:5])
            for k in ('mean_error', 'mean_error_procrustes', 'mean_auc', 'mean_pck'):
                assert np.isfinite(ref[k]) and abs(got[k] - ref[k]) < 1e-4 * max(1.0, abs(ref[k])), (n, seed, k, got[k], ref[k])
            if masked and nj > 3:
                assert np.isnan(ref['auc'][1]) and np.isnan(ref['pck'][1]) and np.isnan(got['auc'][1]) and np.isnan(got['pck'][1])
            assert np.array_equal(np.isnan(got['auc']), np.isnan(ref['auc'])) and np.array_equal(np.isnan(got['pck']), np.isnan(ref['pck']))
            assert np.allclose(got['auc'], ref['auc'], atol=1e-5, equal_nan=True), (n, seed)
            assert np.allclose(got['pck'], ref['pck'], atol=1e-6, equal_nan=True), (n, seed)
    print(f'{nj} joints, masked {masked}: worst |dist_procrustes - oracle| per family (mm): '
          + ', '.join(f'{f} {w:.1e}' for f, w in zip(FAMILIES, worst)))


@pytest.mark.gpu
def test_hip_metrics_where_the_alignment_is_not_unique(cuda):
    """Exactly collinear truth and two valid joints: the optimal rotation is not unique, so the aligned distance is whatever
    the SVD at hand picks.  What IS defined is asserted: the plain distance, PCK and AUC as everywhere else, and
    dist_procrustes finite exactly where the oracle's is -- everywhere: LAPACK completes a rank-1 fit with SOME rotation, and
    on one valid joint (both centred sets are 0, A is 0 / 0) its SVD raises and the reference keeps the prediction
    (util3d.py:152-154), so there dist_procrustes equals dist.  Until this test eval_pose_kernel's arithmetic had no answer for either case
    (A v / 0 for a singular value that is exactly 0; 0 / 0 for a zero-norm set), and one NaN is enough to turn
    mean_error_procrustes of a whole evaluation into NaN."""
    rng = np.random.default_rng(9)
    n, nj = 130, 17
    pred, true, _ = _family_poses(n, nj, 0)
    true[:40] = (rng.standard_normal((40, nj, 1)) * 250 * rng.standard_normal((40, 1, 3))).astype(np.float32)   # on a line
    true[:10, :, 1:] = 0                                                                          # ... an axis
    valid = np.ones((n, nj), bool)
    valid[40:80] = False
    valid[40:80, 3] = True                                                                        # one valid joint
    valid[80:, 2:] = False                                                                        # two valid joints
    with np.errstate(invalid='ignore', divide='ignore'):
        ref = oracle_metrics(pred, true, valid)
    got = _gpu_metrics(cuda, pred, true, valid)
    assert np.abs(got['dist'] - ref['dist']).max() < 1e-3
    assert np.isfinite(ref['dist_procrustes']).all() and np.array_equal(ref['dist_procrustes'][40:80], ref['dist'][40:80])
    assert np.abs(got['dist_procrustes'][40:80] - ref['dist_procrustes'][40:80]).max() < 2e-3
    assert np.isfinite(got['mean_error_procrustes'])
    assert np.array_equal(np.isfinite(got['dist_procrustes']), np.isfinite(ref['dist_procrustes'])), \
        np.flatnonzero((np.isfinite(got['dist_procrustes']) != np.isfinite(ref['dist_procrustes'])).any(axis=1))
    for k in ('mean_error', 'mean_auc', 'mean_pck'):
        assert abs(got[k] - ref[k]) < 1e-4 * max(1.0, abs(ref[k])), k
    assert np.allclose(got['auc'], ref['auc'], atol=1e-5, equal_nan=True) and np.allclose(got['pck'], ref['pck'], atol=1e-6, equal_nan=True)
