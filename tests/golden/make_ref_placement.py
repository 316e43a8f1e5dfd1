#!/usr/bin/env python3
"""Absolute poses and frame keypoints computed BY THE REFERENCE'S OWN CODE, from a checkout of isarandi/metro-pose3d:

    python tests/golden/make_ref_placement.py REFERENCE_CHECKOUT      # writes tests/golden/ref_placement_v1.npz

The reference's camera code (src/cameralib.py: support_single, class Camera, look_at_box, reproject_image_points,
reproject_image_points_fast, project_points without its numba decorator, allclose_or_nones) and its z-offset solve
(src/model/bone_length_based_backproj.py: optimize_z_offset_by_bones_single, scipy's least_squares) are cut out of their files
with `ast` and executed, as tests/golden/make_ref_frames.py does (cv2 substituted the same way).  The TensorFlow lines of the
test path are restated in NumPy on fp32 tensors, each next to its source line:
  heatmap_to_image             src/model/volumetric.py:288-295
  inv_intrinsics einsum        volumetric.py:174-175, 221-222 (matmul_joint_coords: 'Bij,BCj->BCi')
  delta_z                      volumetric.py:176
  back_project                 volumetric.py:284-285
  to_orig_cam (+ cam_loc)      volumetric.py:202-208, 277-281
  inv_intrinsics, rot_to_orig_cam, rot_to_world, cam_loc       src/data/data_loading.py:110-112, 119
Keypoints go through reproject_image_points' GENERAL branch, orig.world_to_image(virt.image_to_world(p)) (cameralib.py:
258-259), evaluated with image_to_world's camera_depth = 4000 mm instead of its default 1: at depth 1 the fp32 world round
trip cancels against the camera centre (|t| ~ 5 m: 0.4 px; stored as `keypoints_depth1`).  Its fast branch
(reproject_image_points_fast, :432-438), which the dispatcher takes for undistorted cameras and [N, 2] points, maps in the opposite direction to its docstring (H = old new^-1).  `fast_keypoints` records what that branch
returns for the same points, called as the dispatcher would (points, virtual, original), as evidence of the finding.

Inputs: the three cameras and 20 boxes of ref_frames_v1.npz; per box a synthetic H36M-order pose (17 head joints, root last)
seen by the box's virtual camera, turned into soft-argmax coordinates in [0, 1] (with noise), per-box bone-length targets over
the head edges and root depths.  Outputs: the virtual K^-1, the rotations, cam_loc, the crop -> frame keypoints and the poses
of the three scale recoveries in crop / camera / world coordinates, head order.  `metro` is the engine's meaning (the
root-relative heatmap_to_metric pose, rotated; no cam_loc).  No source text is stored.
"""
from __future__ import annotations

import copy
import functools
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np
import scipy.optimize

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests.golden import make_ref_frames as MRF  # noqa: E402
from metro_pose3d_amd.joints import skeleton  # noqa: E402

OUT = os.path.join(HERE, 'ref_placement_v1.npz')
FRAMES = os.path.join(HERE, 'ref_frames_v1.npz')
SIDE, STRIDE, BOX_MM, CENTERED = 256, 32, 2200.0, True

# a standing person, mm, camera-like axes (x right, y down, z away), head order of joints.py _H36M_HEAD (pelvis last)
TEMPLATE = np.array([
    [-130, 0, 0], [-140, 440, 30], [-150, 880, 0], [130, 0, 0], [140, 440, -20], [150, 880, 10],
    [0, -230, 10], [0, -480, 0], [0, -560, -30], [0, -700, -10], [170, -450, 0], [260, -200, 40], [300, 30, 80],
    [-170, -450, 0], [-270, -210, -30], [-320, 20, -60], [0, 0, 0]], np.float64)


def heatmap_to_image(coords):                       # volumetric.py:288-295 on fp32
    last = SIDE - 1
    lrc = last - (last % STRIDE) - 1
    out = coords * np.float32(lrc)
    if CENTERED:
        out = out + np.float32(STRIDE // 2)
    return out.astype(np.float32)


def to_orig_cam(x, rot, mirror):                    # volumetric.py:277-281
    y = np.einsum('Bij,BCj->BCi', rot, x).astype(np.float32)
    det = np.linalg.det(rot.astype(np.float64))
    return np.where((det > 0)[:, None, None], y, y[:, mirror])


def main(ref):
    MRF.REF = ref
    cv2 = MRF.Cv2()
    ns = {'np': np, 'copy': copy, 'functools': functools, 'cv2': cv2}
    MRF.cut('src/boxlib.py', ['center'], ns)
    ns['boxlib'] = types.SimpleNamespace(center=ns['center'])
    MRF.cut('src/cameralib.py', ['support_single', 'Camera', 'look_at_box', 'reproject_image_points',
                                 'reproject_image_points_fast', 'project_points', 'allclose_or_nones'], ns,
            strip_decorators=('project_points',))
    nsb = {'np': np, 'scipy': scipy, 'tf': None, 'tfu': None}
    MRF.cut('src/model/bone_length_based_backproj.py', ['optimize_z_offset_by_bones_single'], nsb)
    Camera, look_at_box = ns['Camera'], ns['look_at_box']
    solve = nsb['optimize_z_offset_by_bones_single']

    fr = np.load(FRAMES)
    cams = []
    for i in range(3):
        dist = fr[f'cam{i}_dist']
        cams.append(Camera(fr[f'cam{i}_t'], fr[f'cam{i}_r'], fr[f'cam{i}_k'], dist if dist.size else None,
                           world_up=tuple(fr[f'cam{i}_world_up'].tolist())))
    boxes, box_camera = fr['boxes'], fr['box_camera']
    n = len(boxes)
    sk = skeleton('h36m')
    edges = np.asarray(sk.head_edges, np.int32)
    mirror = np.asarray(sk.head_mirror, np.int32)
    rng = np.random.default_rng(20261015)
    last = SIDE - 1
    lrc = last - (last % STRIDE) - 1

    rec = {k: [] for k in ('inv_k', 'rot_to_orig_cam', 'rot_to_world', 'cam_loc', 'coords01', 'keypoints', 'keypoints_depth1',
                           'fast_keypoints')}
    depth_true, bones = [], []
    for i in range(n):
        orig = cams[box_camera[i]]
        virt = look_at_box(orig, boxes[i], SIDE)
        # the person: the template turned about the vertical axis, its pelvis 3-6 m in front of the virtual camera
        a = rng.uniform(-np.pi, np.pi)
        rot_y = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        z_root = rng.uniform(3000, 6000)
        x = TEMPLATE @ rot_y.T + [0, -150, z_root]
        uv = x[:, :2] / x[:, 2:] @ np.asarray(virt.intrinsic_matrix)[:2, :2].T + np.asarray(virt.intrinsic_matrix)[:2, 2]
        c01 = np.concatenate([(uv - STRIDE // 2) / lrc, ((x[:, 2] - z_root) / BOX_MM + 0.5)[:, None]], axis=1)
        c01 = c01 + rng.normal(0, [0.002, 0.002, 0.004], c01.shape)
        rec['coords01'].append(c01.astype(np.float32))
        bl = np.linalg.norm(x[edges[:, 0]] - x[edges[:, 1]], axis=1)
        bones.append(bl * (1 + rng.normal(0, 0.03, bl.shape)))
        depth_true.append(z_root)
        rec['inv_k'].append(np.linalg.inv(virt.intrinsic_matrix).astype(np.float32))    # data_loading.py:112
        rec['rot_to_orig_cam'].append((orig.R @ virt.R.T).astype(np.float32))           # :110
        rec['rot_to_world'].append(virt.R.T.astype(np.float32))                         # :111
        rec['cam_loc'].append(virt.t.astype(np.float32))                                # :119
        im2d = heatmap_to_image(rec['coords01'][-1][:, :2])
        # cameralib.py:258-259 at camera_depth 4000 mm: at the default depth 1 the fp32 world round trip cancels against
        # |t| (~5 m for cameras 0 and 1: 5e-4 relative, 0.4 px); `keypoints_depth1` keeps that answer for the record
        rec['keypoints'].append(orig.world_to_image(virt.image_to_world(im2d, camera_depth=4000)).astype(np.float32))
        rec['keypoints_depth1'].append(orig.world_to_image(virt.image_to_world(im2d)).astype(np.float32))
        rec['fast_keypoints'].append(np.asarray(ns['reproject_image_points_fast'](im2d, virt, orig), np.float32))
    out = {k: np.stack(v) for k, v in rec.items()}
    coords01 = out['coords01']
    bone_lengths = np.stack(bones)
    root_depth = (np.asarray(depth_true) * (1 + rng.normal(0, 0.01, n))).astype(np.float32)

    # the test path on fp32 tensors (volumetric.py:171-208)
    im2d = heatmap_to_image(coords01[..., :2])
    homog = np.concatenate([im2d, np.ones_like(im2d[..., :1])], axis=-1)
    cam = np.einsum('Bij,BCj->BCi', out['inv_k'], homog).astype(np.float32)
    delta_z = ((coords01[..., 2] - coords01[:, -1:, 2]) * np.float32(BOX_MM)).astype(np.float32)
    z_bones = np.array([solve(cam[i], delta_z[i], bone_lengths[i], edges) for i in range(n)], np.float32)
    for name, z in (('bone_lengths', z_bones), ('true_root_depth', root_depth)):
        crop = (cam * (delta_z + z[:, None])[..., None]).astype(np.float32)                # back_project
        out[f'{name}_crop'] = crop
        out[f'{name}_camera'] = to_orig_cam(crop, out['rot_to_orig_cam'], mirror)
        out[f'{name}_world'] = (to_orig_cam(crop, out['rot_to_world'], mirror) + out['cam_loc'][:, None]).astype(np.float32)
        out[f'{name}_z_offset'] = z
    metric = np.concatenate([im2d * np.float32(BOX_MM) / np.float32(SIDE), coords01[..., 2:] * np.float32(BOX_MM)], -1)
    metro = (metric - metric[:, -1:]).astype(np.float32)                                   # tfu3d.py:23-25
    out.update(metro_crop=metro, metro_camera=to_orig_cam(metro, out['rot_to_orig_cam'], mirror),
               metro_world=to_orig_cam(metro, out['rot_to_world'], mirror))
    out.update(boxes=boxes, box_camera=box_camera, bone_targets=bone_lengths, root_depth=root_depth, edges=edges,
               mirror=mirror, side=np.int32(SIDE), stride=np.int32(STRIDE), box_size_mm=np.float32(BOX_MM))
    np.savez_compressed(OUT, **out)
    print(f'wrote {OUT}: {n} boxes, {os.path.getsize(OUT)} bytes; z offsets {z_bones.min():.0f} .. {z_bones.max():.0f} mm')


if __name__ == '__main__':
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], 'src', 'cameralib.py')):
        raise SystemExit('usage: make_ref_placement.py REFERENCE_CHECKOUT (the directory holding src/cameralib.py)')
    main(os.path.abspath(sys.argv[1]))
