"""CPU restatement of metro_place_poses (metro_pose3d_amd/csrc/place_poses.hip): absolute poses and frame keypoints of frame
crops.  TEST INFRASTRUCTURE: built on oracle/heads.py (the reference's back-projection and its scipy z-offset solve) and
tests/oracle_frames.py (project_points).  The product never imports it.

Everything here is in the kernel's output joint order: `perm` maps output rows to head joints, `mirror` is the output-order
mirror table (Skeleton.out_mirror)."""
from __future__ import annotations

import numpy as np

from oracle import heads as OH
from tests import oracle_frames as OP

SCALES = ('metro', 'bone-lengths', 'true-root-depth')
COORDS = ('crop', 'camera', 'world')


def place(coords01, params, stride, scale, coords, perm, mirror, edges=None, bone_lengths=None, root_depth=None,
          poses_rel=None, proc_side=256, centered=True, box_size_mm=2200.0):
    """coords01 fp32 [n, J_head, 3]; params: frames.PlacementParams.  Returns (poses [n, Jout, 3], keypoints [n, Jout, 2],
    z_offset [n] or None).  poses_rel: the engine's root-relative poses [n, Jout, 3] (scale 'metro')."""
    c = np.asarray(coords01, np.float32)
    perm = list(perm)
    z = None
    if scale == 'metro':
        x = np.asarray(poses_rel, np.float32)
    else:
        cam, dz = OH.camcoords_and_delta_z(c, params.inv_intrinsics, stride, proc_side, centered, box_size_mm)
        if scale == 'bone-lengths':
            t = np.asarray(bone_lengths, np.float64)
            z = np.array([OH.optimize_z_offset_by_bones_single(cam[i], dz[i], t if t.ndim == 1 else t[i], edges)
                          for i in range(len(c))], np.float32)
        else:
            z = np.asarray(root_depth, np.float32)
        x = OH.back_project(cam, dz, z)[:, perm]
    if coords == 'camera':
        x = OH.to_orig_cam(x, params.rot_to_orig_cam, mirror)
    elif coords == 'world':
        x = OH.to_orig_cam(x, params.rot_to_world, mirror)
        if scale != 'metro':
            x = (x + params.cam_loc[:, None]).astype(np.float32)
    return x, keypoints(c, params, stride, perm, proc_side, centered), z


def keypoints(coords01, params, stride, perm, proc_side=256, centered=True):
    """heatmap_to_image(coords01.xy) in output order, mapped into the frame: the crop -> frame homography, or
    rot_to_orig_cam . K^-1 . (u, v, 1) and project_points; NaN behind the original camera."""
    uv = OH.heatmap_to_image(np.asarray(coords01, np.float32)[:, perm, :2], stride, proc_side, centered)
    out = np.full(uv.shape, np.nan, np.float32)
    f32 = np.float32
    for i in range(len(uv)):
        h = np.concatenate([uv[i], np.ones_like(uv[i][:, :1])], axis=1)
        if params.keypoint_mode[i] == 1:             # METRO_WARP_DISTORTED
            k = params.inv_intrinsics[i]
            r = params.rot_to_orig_cam[i]
            cam = np.stack([(k[j, 0] * h[:, 0] + k[j, 1] * h[:, 1]) + k[j, 2] * f32(1) for j in range(3)], -1)
            ray = np.stack([(r[j, 0] * cam[:, 0] + r[j, 1] * cam[:, 1]) + r[j, 2] * cam[:, 2] for j in range(3)], -1)
            ok = ray[:, 2] > 0
            u, v = OP.project_points(ray[ok].astype(np.float32), params.intrinsics[i], params.distortion[i])
            out[i][ok] = np.stack([u, v], -1)
        else:
            hm = params.homography[i]
            p = np.stack([(hm[j, 0] * h[:, 0] + hm[j, 1] * h[:, 1]) + hm[j, 2] for j in range(3)], -1).astype(np.float32)
            ok = p[:, 2] > 0
            out[i][ok] = p[ok, :2] / p[ok, 2:]
    return out
