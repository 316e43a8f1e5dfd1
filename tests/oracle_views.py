"""NumPy restatement of metro_merge_views (metro_pose3d_amd/csrc/views.hip): the V views of each box fused into one result.
TEST INFRASTRUCTURE: the product never imports it."""
from __future__ import annotations

import numpy as np


def merge(poses, keypoints, z_offset, rot_to_orig_cam, mirror, n_views: int):
    """poses fp32 [n V, J, 3] (placed, joints already mirrored); keypoints fp32 [n V, J, 2] (unmirrored) or None; z_offset
    [n V] or None; rot_to_orig_cam fp32 [n V, 3, 3] of the views' records; mirror [J] output-order mirror joints.
    Returns (poses [n, J, 3], keypoints [n, J, 2] or None, z [n] or None, spread [n, J]), all float32: fp64 means over the
    views (keypoints: over the finite ones, a view with det <= 0 contributing its mirror joint's, NaN if none), spread the RMS
    3D distance of the views from their mean."""
    p = np.asarray(poses, np.float64)
    nv = int(n_views)
    n, nj = len(p) // nv, p.shape[1]
    p = p.reshape(n, nv, nj, 3)
    mean = p.sum(axis=1) / nv
    d = p - mean[:, None]
    spread = np.sqrt((d * d).sum(axis=-1).sum(axis=1) / nv)
    kp_out = z_out = None
    if keypoints is not None:
        k = np.asarray(keypoints, np.float64).reshape(n, nv, nj, 2)
        det = np.linalg.det(np.asarray(rot_to_orig_cam, np.float64)).reshape(n, nv)
        k = np.where(~(det > 0)[:, :, None, None], k[:, :, np.asarray(mirror)], k)
        ok = np.isfinite(k).all(axis=-1)
        cnt = ok.sum(axis=1)
        s = np.where(ok[..., None], k, 0.0).sum(axis=1)
        with np.errstate(invalid='ignore', divide='ignore'):
            kp_out = np.where(cnt[..., None] > 0, s / cnt[..., None], np.nan).astype(np.float32)
    if z_offset is not None:
        z_out = (np.asarray(z_offset, np.float64).reshape(n, nv).sum(axis=1) / nv).astype(np.float32)
    return mean.astype(np.float32), kp_out, z_out, spread.astype(np.float32)
