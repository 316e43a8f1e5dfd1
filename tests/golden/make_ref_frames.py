#!/usr/bin/env python3
"""Virtual cameras and warp maps computed BY THE REFERENCE ITSELF, from a checkout of isarandi/metro-pose3d:

    python tests/golden/make_ref_frames.py REFERENCE_CHECKOUT        # writes tests/golden/ref_frames_v1.npz

The reference's camera code (src/cameralib.py: support_single, class Camera, look_at_box, reproject_image,
reproject_image_fast, get_grid_coords, project_points without its numba decorator, allclose_or_nones), boxlib.center
(src/boxlib.py:14-15) and make_3dhp_test_camera (src/data/mpi_inf_3dhp.py:260-269) are cut out of their files with `ast` and
executed with NumPy.  Only the cv2 calls are substituted: undistortPoints by the restatement in tests/oracle_frames.py,
convertPointsToHomogeneous by appending a 1 (float32 stays float32), and remap by a recorder that keeps the float32 maps the
reference hands to it (the sampling itself is pinned elsewhere: tests/test_preprocess.py).
Three cameras: an H36M-like one (k1 ~ -0.2, non-zero tangential terms; src/data/h36m.py:222-233 builds it the same way), the
3DHP test camera 5/6 (mpi_inf_3dhp.py:114-121, with its distortion coefficients) and an intrinsics-only one (no distortion:
the reference's fast path).  Stored: inputs, the virtual K and R of look_at_box, the rotations back (data_loading.py:
110-111) and a 33 x 33 subgrid of each crop's remap coordinates.  No source text is stored.
"""
from __future__ import annotations

import ast
import copy
import functools
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.oracle_frames import undistort_points  # noqa: E402

REF = None                  # the reference checkout (command line)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'ref_frames_v1.npz')
SIDE = 256
SUB = np.r_[0:SIDE:8, SIDE - 1]


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
    BORDER_CONSTANT, INTER_LINEAR, INTER_AREA, WARP_INVERSE_MAP = 0, 1, 3, 16

    def __init__(self):
        self.maps = None

    @staticmethod
    def undistortPoints(points, k, dist, r=None, p=None, *_):           # noqa: N802
        assert r is None and p is None
        return undistort_points(np.asarray(points).reshape(-1, 2), k, dist).reshape(1, -1, 2)

    @staticmethod
    def convertPointsToHomogeneous(points):                             # noqa: N802
        p = np.asarray(points).reshape(-1, 2)
        return np.concatenate([p, np.ones_like(p[:, :1])], axis=1)[:, None, :]

    def remap(self, image, map1, map2, interp, borderMode=None, borderValue=None):   # noqa: N803
        assert interp == self.INTER_LINEAR and borderMode == self.BORDER_CONSTANT and borderValue == 0
        self.maps = np.stack([map1[..., 0], map1[..., 1]]) if map2 is None else np.stack([map1, map2])
        assert self.maps.dtype == np.float32
        return np.zeros(self.maps.shape[1:] + image.shape[2:], image.dtype)

    @staticmethod
    def warpAffine(*args, **kwargs):                                    # noqa: N802
        raise AssertionError('case 1 of reproject_image is not part of the fixture')


def rot_looking(forward, up=(0., 0., 1.), roll_deg=0.):
    z = np.asarray(forward, np.float64)
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    a = np.deg2rad(roll_deg)
    return np.stack([np.cos(a) * x + np.sin(a) * y, -np.sin(a) * x + np.cos(a) * y, z])


def main():
    cv2 = Cv2()
    ns = {'np': np, 'copy': copy, 'functools': functools, 'cv2': cv2}
    cut('src/boxlib.py', ['center'], ns)
    ns['boxlib'] = types.SimpleNamespace(center=ns['center'])
    cut('src/cameralib.py', ['support_single', 'Camera', 'look_at_box', 'reproject_image', 'reproject_image_fast',
                             'get_grid_coords', 'project_points', 'allclose_or_nones'], ns, strip_decorators=('project_points',))
    Camera = ns['Camera']
    ns3 = {'np': np, 'cameralib': types.SimpleNamespace(Camera=Camera)}
    cut('src/data/mpi_inf_3dhp.py', ['make_3dhp_test_camera'], ns3)

    k_h36m = np.array([[1145.05, 0, 512.54], [0, 1143.78, 515.45], [0, 0, 1]], np.float32)
    cameras = [
        # H36M-like: Camera(t, R, K, dist) as make_h36m_camera does, world_up (0, 0, 1)
        (Camera(np.array([1841.1, 4955.3, 1563.4]), rot_looking((-0.35, -0.93, -0.12), roll_deg=1.5), k_h36m,
                np.array([-0.2071, 0.2479, -0.00142, -0.00098, -0.00309], np.float32)), (1002, 1000)),
        # 3DHP test camera 5/6 (mpi_inf_3dhp.py:114-121), world_up (0, 1, 0)
        (ns3['make_3dhp_test_camera'](
            sensor_size=np.array([10, 5.625]), im_size=np.array([1920, 1080]), focal_length=8.770747185,
            pixel_aspect=0.993236423, center_offset=np.array([-0.104908645, 0.104899704]),
            distortion=np.array([-0.276859611, 0.131125256, -0.000360494, -0.001149441, -0.049318332]),
            origin=np.array([-2104.3074, 1038.6707, -4596.6367]), up=np.array([0.025272345, 0.995038509, 0.096227370]),
            right=np.array([-0.939647257, -0.009210289, 0.342020929])), (1080, 1920)),
        # intrinsics only (R = I, t = 0), world_up (0, -1, 0) as metro_pose3d_amd.frames.Camera defaults to
        (Camera(intrinsic_matrix=np.array([[1000., 0, 640], [0, 1002, 360], [0, 0, 1]]), world_up=(0, -1, 0)), (720, 1280)),
    ]
    boxes = [  # (camera, x, y, w, h): inside, partly outside, near the corners, wide and tall
        (0, 400, 300, 200, 450), (0, 0, 0, 150, 300), (0, -60, 500, 200, 400), (0, 880, 850, 160, 200),
        (0, 300, 600, 400, 150), (0, 700, 200, 60, 120), (0, 470, 430, 90, 160),
        (1, 900, 300, 220, 520), (1, 0, 0, 200, 400), (1, 1800, 900, 250, 300), (1, -100, 600, 300, 420),
        (1, 1500, 100, 180, 160), (1, 600, 700, 500, 300), (1, 1850, -40, 120, 260),
        (2, 590, 260, 100, 200), (2, 0, 0, 200, 300), (2, 1150, 600, 200, 200), (2, -50, 400, 180, 380),
        (2, 800, 100, 300, 120), (2, 300, 500, 90, 240),
    ]
    rec = {k: [] for k in ('virt_k', 'virt_r', 'rot_to_orig_cam', 'rot_to_world', 'maps')}
    for c, *box in boxes:
        cam, (h, w) = cameras[c]
        box = np.array(box, np.float64)
        virt = ns['look_at_box'](cam, box, SIDE)
        ns['reproject_image'](np.zeros((h, w, 3), np.uint8), cam, virt, (SIDE, SIDE))
        rec['virt_k'].append(np.asarray(virt.intrinsic_matrix, np.float64))
        rec['virt_r'].append(virt.R)
        rec['rot_to_orig_cam'].append((cam.R @ virt.R.T).astype(np.float32))
        rec['rot_to_world'].append(virt.R.T.astype(np.float32))
        rec['maps'].append(cv2.maps[:, SUB][:, :, SUB])
    out = {k: np.stack(v) for k, v in rec.items()}
    out.update(boxes=np.array([b[1:] for b in boxes], np.float64), box_camera=np.array([b[0] for b in boxes], np.int32),
               subgrid=SUB, side=np.int32(SIDE))
    for i, (cam, (h, w)) in enumerate(cameras):
        out.update({f'cam{i}_k': cam.intrinsic_matrix, f'cam{i}_r': cam.R, f'cam{i}_t': cam.t,
                    f'cam{i}_world_up': np.asarray(cam.world_up), f'cam{i}_frame_hw': np.array([h, w], np.int32),
                    f'cam{i}_dist': (np.zeros(0, np.float32) if cam.distortion_coeffs is None else cam.distortion_coeffs)})
    np.savez_compressed(OUT, **out)
    print(f'wrote {OUT}: {len(boxes)} boxes, {os.path.getsize(OUT)} bytes')


if __name__ == '__main__':
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], 'src', 'cameralib.py')):
        raise SystemExit('usage: make_ref_frames.py REFERENCE_CHECKOUT (the directory holding src/cameralib.py)')
    REF = os.path.abspath(sys.argv[1])
    main()
