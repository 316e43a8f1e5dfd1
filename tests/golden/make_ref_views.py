#!/usr/bin/env python3
"""Test-time view cameras computed BY THE REFERENCE ITSELF, from a checkout of isarandi/metro-pose3d:

    python tests/golden/make_ref_views.py REFERENCE_CHECKOUT        # writes tests/golden/ref_views_v1.npz

The reference's camera code (src/cameralib.py: support_single, class Camera with its zoom, rotate and horizontal_flip,
look_at_box, project_points without its numba decorator) and boxlib.center are cut out of their files with `ast` and executed
with NumPy, as tests/golden/make_ref_frames.py does.  Substituted: the cv2 calls (undistortPoints by the restatement in
tests/oracle_frames.py, convertPointsToHomogeneous by appending a 1) and transforms3d.euler.euler2mat, by the restatement of
transforms3d's published algorithm below (the axis-code table, first axis / parity / repetition / frame, and the entry
formulas).  The cameras are the three of tests/golden/ref_frames_v1.npz, rebuilt from its stored inputs with the reference's
own Camera.  Each view is the loader's --test-aug sequence (src/data/data_loading.py:60-68, 77): look_at_box, zoom, rotate(roll),
horizontal_flip; the records are the loader's rot_to_orig_cam = orig.R cam.R^T, rot_to_world = cam.R^T and
inv(cam.intrinsic_matrix), cast to float32 (:110-112).  Also stored: Camera.rotate with all three angles and
Camera.horizontal_flip on the first camera.  No source text is stored.
"""
from __future__ import annotations

import ast
import copy
import functools
import math
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.oracle_frames import undistort_points  # noqa: E402

REF = None
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'ref_views_v1.npz')
FRAMES_FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'ref_frames_v1.npz')
SIDE = 256
VIEWS = [(0.0, 1.0, False), (-20.0, 1.0, False), (-10.0, 1.0, True), (7.5, 1.2, False), (20.0, 0.8, True), (0.0, 1.0, True),
         (13.0, 1.25, False)]
BOXES = [0, 3, 7, 12, 14, 17]                      # two boxes per camera of the frames fixture
ANGLES = [(0.3, 0.0, 0.0), (0.0, -0.4, 0.0), (0.0, 0.0, 0.5), (0.2, -0.3, 0.7), (-1.1, 0.6, -2.0)]   # (yaw, pitch, roll)


def cut(relpath, names, ns, strip_decorators=()):
    path = os.path.join(REF, relpath)
    tree = ast.parse(open(path).read())
    nodes = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert sorted(n.name for n in nodes) == sorted(names), (relpath, names)
    for n in nodes:
        if n.name in strip_decorators:
            n.decorator_list = []
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, 'exec'), ns)
    return ns


class Cv2:
    @staticmethod
    def undistortPoints(points, k, dist, r=None, p=None, *_):           # noqa: N802
        assert r is None and p is None
        return undistort_points(np.asarray(points).reshape(-1, 2), k, dist).reshape(1, -1, 2)

    @staticmethod
    def convertPointsToHomogeneous(points):                             # noqa: N802
        p = np.asarray(points).reshape(-1, 2)
        return np.concatenate([p, np.ones_like(p[:, :1])], axis=1)[:, None, :]


# transforms3d.euler (after Gohlke's transformations.py): axis code -> (first axis, parity, repetition, frame)
_AXES2TUPLE = {
    'sxyz': (0, 0, 0, 0), 'sxyx': (0, 0, 1, 0), 'sxzy': (0, 1, 0, 0), 'sxzx': (0, 1, 1, 0), 'syzx': (1, 0, 0, 0),
    'syzy': (1, 0, 1, 0), 'syxz': (1, 1, 0, 0), 'syxy': (1, 1, 1, 0), 'szxy': (2, 0, 0, 0), 'szxz': (2, 0, 1, 0),
    'szyx': (2, 1, 0, 0), 'szyz': (2, 1, 1, 0), 'rzyx': (0, 0, 0, 1), 'rxyx': (0, 0, 1, 1), 'ryzx': (0, 1, 0, 1),
    'rxzx': (0, 1, 1, 1), 'rxzy': (1, 0, 0, 1), 'ryzy': (1, 0, 1, 1), 'rzxy': (1, 1, 0, 1), 'ryxy': (1, 1, 1, 1),
    'ryxz': (2, 0, 0, 1), 'rzxz': (2, 0, 1, 1), 'rxyz': (2, 1, 0, 1), 'rzyz': (2, 1, 1, 1)}
_NEXT_AXIS = [1, 2, 0, 1]


def euler2mat(ai, aj, ak, axes='sxyz'):
    firstaxis, parity, repetition, frame = _AXES2TUPLE[axes]
    i = firstaxis
    j = _NEXT_AXIS[i + parity]
    k = _NEXT_AXIS[i - parity + 1]
    if frame:
        ai, ak = ak, ai
    if parity:
        ai, aj, ak = -ai, -aj, -ak
    si, sj, sk = math.sin(ai), math.sin(aj), math.sin(ak)
    ci, cj, ck = math.cos(ai), math.cos(aj), math.cos(ak)
    cc, cs = ci * ck, ci * sk
    sc, ss = si * ck, si * sk
    m = np.eye(3)
    if repetition:
        m[i, i], m[i, j], m[i, k] = cj, sj * si, sj * ci
        m[j, i], m[j, j], m[j, k] = sj * sk, -cj * ss + cc, -cj * cs - sc
        m[k, i], m[k, j], m[k, k] = -sj * ck, cj * sc + cs, cj * cc - ss
    else:
        m[i, i], m[i, j], m[i, k] = cj * ck, sj * sc - cs, sj * cc + ss
        m[j, i], m[j, j], m[j, k] = cj * sk, sj * ss + cc, sj * cs - sc
        m[k, i], m[k, j], m[k, k] = -sj, cj * si, cj * ci
    return m


def main():
    ns = {'np': np, 'copy': copy, 'functools': functools, 'cv2': Cv2(),
          'transforms3d': types.SimpleNamespace(euler=types.SimpleNamespace(euler2mat=euler2mat))}
    cut('src/boxlib.py', ['center'], ns)
    ns['boxlib'] = types.SimpleNamespace(center=ns['center'])
    cut('src/cameralib.py', ['support_single', 'Camera', 'look_at_box', 'project_points'], ns,
        strip_decorators=('project_points',))
    Camera = ns['Camera']
    fr = np.load(FRAMES_FIX)
    cams = []
    for i in range(3):
        dist = fr[f'cam{i}_dist']
        cams.append(Camera(fr[f'cam{i}_t'], fr[f'cam{i}_r'], fr[f'cam{i}_k'], dist if dist.size else None,
                           world_up=tuple(fr[f'cam{i}_world_up'].tolist())))
    rec = {k: [] for k in ('view_k', 'view_r', 'rot_to_orig_cam', 'rot_to_world', 'inv_k')}
    for b in BOXES:
        orig = cams[fr['box_camera'][b]]
        for roll_deg, zoom, flip in VIEWS:
            cam = ns['look_at_box'](orig, fr['boxes'][b], SIDE)
            cam.zoom(zoom)
            cam.rotate(roll=roll_deg * np.pi / 180)
            if flip:
                cam.horizontal_flip()
            rec['view_k'].append(np.asarray(cam.intrinsic_matrix, np.float64))
            rec['view_r'].append(np.asarray(cam.R, np.float64))
            rec['rot_to_orig_cam'].append((orig.R @ cam.R.T).astype(np.float32))
            rec['rot_to_world'].append(cam.R.T.astype(np.float32))
            rec['inv_k'].append(np.linalg.inv(cam.intrinsic_matrix).astype(np.float32))
    out = {k: np.stack(v) for k, v in rec.items()}
    rotated = []
    for yaw, pitch, roll in ANGLES:
        cam = cams[0].copy()
        cam.rotate(yaw=yaw, pitch=pitch, roll=roll)
        rotated.append(np.asarray(cam.R, np.float64))
    flipped = cams[0].copy()
    flipped.horizontal_flip()
    out.update(boxes=np.asarray(BOXES, np.int32), views_roll_deg=np.array([v[0] for v in VIEWS]),
               views_zoom=np.array([v[1] for v in VIEWS]), views_flip=np.array([v[2] for v in VIEWS]),
               angles=np.asarray(ANGLES, np.float64), rotated_r=np.stack(rotated), flipped_r=np.asarray(flipped.R),
               side=np.int32(SIDE))
    np.savez_compressed(OUT, **out)
    print(f'wrote {OUT}: {len(BOXES)} boxes x {len(VIEWS)} views, {os.path.getsize(OUT)} bytes')


if __name__ == '__main__':
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], 'src', 'cameralib.py')):
        raise SystemExit('usage: make_ref_views.py REFERENCE_CHECKOUT (the directory holding src/cameralib.py)')
    REF = os.path.abspath(sys.argv[1])
    main()
