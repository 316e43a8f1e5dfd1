"""Pose estimation on full camera frames: person boxes and (optionally calibrated, lens-distorted) cameras in, poses out.

The reference's test path (src/data/data_loading.py:33-58, 107-111) builds a virtual camera per person box that turns towards
the box centre, drops the lens distortion, squares the pixels and zooms so the box fills the crop; `cameralib.reproject_image`
(src/cameralib.py:265-324) warps the uint8 frame into it; after the net `volumetric.to_orig_cam` (src/model/volumetric.py:
204-216, 277-281) rotates the poses back into the original camera or the world.  Here:

  Camera, undistort_points, look_at_box   host geometry, the reference's camera restated in its dtypes (fp32 R, K, t)
  crop_params                             per-crop warp mode + matrices and the rotations back (data_loading.py:110-111)
  warp_frames                             one HIP launch (metro_warp_crops_frames_u8) for the crops of many frames
  pixel_format, color_matrix              frames as decoders leave them: 'bgr' (OpenCV), 'nv12' (hardware decoders), 'i420'
                                          (libavcodec's yuv420p), converted per tap inside the warp by
                                          metro_warp_crops_frames_planes; 'rgb' (the default) keeps metro_warp_crops_frames_u8
  estimate_pose_in_frames                 the whole chain on one device, enqueued on the current stream
  placement_params                        per-crop virtual camera (inverse K, rotations, camera centre) and the way back to the
                                          frame's pixels (MetroPlacement records)
  locate_poses_in_frames                  absolute poses (bone-lengths / true-root-depth scale recovery, volumetric.py:171-208)
                                          and 2D frame keypoints, one metro_place_poses launch after the forward
  view_set, pack_view_bases, view_params test-time augmentation (`views=`): V rolled / zoomed / flipped views per box
                                          (data_loading.py:60-68, 77-79), expanded on the device (metro_expand_views) from one
                                          record per box and fused per box after the placement (metro_merge_views)
  look_at_boxes, pack_frame_cameras       the per-box records on the device (metro_look_at_boxes, `geometry='device'`, the
                                          default for CUDA boxes): look_at_box and pack_view_bases restated per thread from a
                                          per-frame camera table, so boxes from a GPU detector stay on the GPU and the call does
                                          no per-box host work ('host' keeps the NumPy geometry and its bits)

Divergences from the reference, on purpose:
  * a Camera built from intrinsics alone (no R, no t) defaults to world_up = (0, -1, 0), not the reference's (0, 0, 1): with
    R = I and t = 0, `turn_towards` takes cross(new_z, (0, 0, 1)), which vanishes for a box near the optical axis;
  * reproject_image's case 1 (cameralib.py:282-293: an all-zero coefficient array whose virtual R is allclose to the original
    goes to cv2.warpAffine, with INTER_AREA when zooming out) is not reproduced: any coefficient array takes the general mode;
  * a general-mode ray that points behind the camera (z <= 0) samples the border value 0; the reference projects it through
    the origin;
  * likewise a keypoint whose ray lies behind the original camera (z <= 0; w <= 0 after the crop -> frame homography) comes
    out of locate_poses_in_frames as NaN; the reference's reproject_image_points projects it through the origin;
  * keypoints of undistorted cameras go through the crop -> frame homography, the mapping the reference's general branch
    `orig.world_to_image(virt.image_to_world(p))` computes; its dispatcher would send them to reproject_image_points_fast
    (cameralib.py:432-438), which maps in the OPPOSITE direction to its docstring (H = old new^-1, i.e. frame -> crop when
    called as (points, virtual, original)): that inverted fast path is not reproduced;
  * test-time views are deterministic (view_set), not the loader's random draws; the loader's `shift_aug_by_rot` centre shift
    is not offered (it would need a look_at_box per view); a flip mirrors about x = side/2, the principal point that
    center_principal_point sets, not about the pixel grid's centre (side - 1)/2;
  * the device geometry (geometry='device') inverts 3x3 matrices in closed form, not with LAPACK's pivoted solves: its records
    are within one fp32 ulp of the host's (most of them bit-identical), not always the host's bits.  The host geometry, the
    default for host boxes, costs ~0.2 ms of NumPy per box and bounds the call there (profiles/frames_probe.json); the
    device geometry takes one ~6 us launch for 64 boxes (profiles/device_geometry_probe.json);
  * a YUV frame ('nv12', 'i420') is the RGB image of OpenCV's integer cvtColor(COLOR_YUV2RGB_NV12 / _I420) rule (limited
    range, BT.601 by default or BT.709, the chroma of each 2x2 block replicated; include/metro_hip.h), not of ffmpeg's
    swscale, which rounds differently; a tap outside the frame is black (RGB 0), not YUV (0, 0, 0).
"""
from __future__ import annotations

import copy
import ctypes as C
import math
import os
from collections import OrderedDict
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from metro_pose3d_amd import _lib
from metro_pose3d_amd._lib import check
from metro_pose3d_amd.preprocess import box_homography

UNDISTORT_ITERATIONS = 5


def undistort_points(points, intrinsic_matrix, distortion_coeffs) -> np.ndarray:
    """cv2.undistortPoints(points, K, D) with R = P = None -> float32 [N, 2] normalised camera coordinates.

    OpenCV is absent here, so this is restated from its published source, modules/imgproc/src/undistort.cpp
    (cvUndistortPoints / cvUndistortPointsInternal, 3.x): K and D converted to double; fx, fy, cx, cy only (a skew term is
    ignored); x = (u - cx) * (1 / fx); with coefficients, the fixed-point iteration
        icdist = 1 / (1 + ((k3 r2 + k2) r2 + k1) r2),  x = (x0 - dx) icdist
    run for the fixed count of the default criteria, TermCriteria(COUNT, 5, 0.01) (`iters = 5` in the older 3.x form), then
    the result is stored as float32 like the float32 input.  PARITY UNPINNED against cv2 itself (no OpenCV to execute)."""
    p = np.asarray(points, np.float32).reshape(-1, 2).astype(np.float64)
    a = np.asarray(intrinsic_matrix, np.float64)
    fx, fy, cx, cy = a[0, 0], a[1, 1], a[0, 2], a[1, 2]
    ifx, ify = 1. / fx, 1. / fy
    x = (p[:, 0] - cx) * ifx
    y = (p[:, 1] - cy) * ify
    if distortion_coeffs is not None:
        k = np.zeros(14)
        d = np.asarray(distortion_coeffs, np.float64).ravel()
        k[:len(d)] = d
        x0, y0 = x, y
        for _ in range(UNDISTORT_ITERATIONS):
            r2 = x * x + y * y
            icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
            delta_x = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2
            delta_y = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2
            x = (x0 - delta_x) * icdist
            y = (y0 - delta_y) * icdist
    return np.stack([x, y], axis=-1).astype(np.float32)


class Camera:
    """The parts of the reference's cameralib.Camera (src/cameralib.py:25-84) the frame pipeline needs, in its dtypes:
    R (world -> camera rotation), t (optical centre in world coordinates) and the intrinsic matrix are float32, the
    distortion coefficients (k1, k2, p1, p2, k3; OpenCV order) float32 or None.

    world_up defaults to (0, 0, 1) like the reference when R or t is given; a camera built from intrinsics alone defaults to
    (0, -1, 0) (image y points down, so "up" is -y): the reference default degenerates there (module docstring)."""

    def __init__(self, intrinsic_matrix, distortion_coeffs=None, R=None, t=None, world_up=None):
        if world_up is None:
            world_up = (0, -1, 0) if R is None and t is None else (0, 0, 1)
        self.R = np.asarray(np.eye(3) if R is None else R, np.float32)
        self.t = np.asarray(np.zeros(3) if t is None else t, np.float32)
        self.intrinsic_matrix = np.asarray(intrinsic_matrix, np.float32)
        self.distortion_coeffs = None if distortion_coeffs is None else np.asarray(distortion_coeffs, np.float32)
        self.world_up = np.asarray(world_up)
        if self.R.shape != (3, 3) or self.t.shape != (3,) or self.intrinsic_matrix.shape != (3, 3):
            raise ValueError('R and intrinsic_matrix must be 3x3, t a 3-vector')
        if not np.allclose(self.intrinsic_matrix[2, :], [0, 0, 1]):
            raise ValueError(f'bottom row of the intrinsic matrix must be (0, 0, 1), got {self.intrinsic_matrix[2, :]}')
        if self.distortion_coeffs is not None and self.distortion_coeffs.shape != (5,):
            raise ValueError(f'distortion_coeffs must be None or 5 values (k1, k2, p1, p2, k3), got '
                             f'{self.distortion_coeffs.shape}')

    def copy(self) -> 'Camera':
        return copy.deepcopy(self)

    # cameralib.py:133-156
    def world_to_camera(self, points):
        return (np.asarray(points, np.float32) - self.t) @ self.R.T

    def camera_to_world(self, points):
        return np.asarray(points, np.float32) @ np.linalg.inv(self.R).T + self.t

    def camera_to_image_undistorted(self, points):
        """camera_to_image (:126-131) of a camera without distortion coefficients."""
        assert self.distortion_coeffs is None
        projected = points[:, :2] / points[:, 2:]
        return projected @ self.intrinsic_matrix[:2, :2].T + self.intrinsic_matrix[:2, 2]

    def image_to_camera(self, points):
        p = undistort_points(points, self.intrinsic_matrix, self.distortion_coeffs)
        return np.concatenate([p, np.ones_like(p[:, :1])], axis=1)        # convertPointsToHomogeneous, depth 1

    def image_to_world(self, points):
        return self.camera_to_world(self.image_to_camera(points))

    # cameralib.py:167-228
    def turn_towards(self, target_image_point):
        target_world_point = self.image_to_world(np.asarray([target_image_point], np.float64))[0]
        new_z = target_world_point - self.t
        new_z = new_z / np.linalg.norm(new_z)
        new_x = np.cross(new_z, self.world_up)
        new_x = new_x / np.linalg.norm(new_x)
        new_y = np.cross(new_z, new_x)
        self.R = np.vstack([new_x, new_y, new_z]).astype(np.float32)

    def undistort(self):
        self.distortion_coeffs = None

    def square_pixels(self):
        fx, fy = self.intrinsic_matrix[0, 0], self.intrinsic_matrix[1, 1]
        fmean = 0.5 * (fx + fy)
        multiplier = np.array([[fmean / fx, 0, 0], [0, fmean / fy, 0], [0, 0, 1]])     # float64, so K becomes float64
        self.intrinsic_matrix = multiplier @ self.intrinsic_matrix

    def zoom(self, factor):
        self.intrinsic_matrix[:2, :2] *= np.expand_dims(factor, -1)

    def center_principal_point(self, imshape):
        self.intrinsic_matrix[:2, 2] = [imshape[1] / 2, imshape[0] / 2]

    # cameralib.py:95-98, 191-192
    def rotate(self, yaw=0, pitch=0, roll=0):
        """R <- euler2mat(yaw, pitch, roll, 'ryxz')^T R (angles in radians): the camera turns by yaw about its y axis, then
        pitch about its new x axis, then roll about its new optical axis.  R becomes float64, as in the reference."""
        self.R = euler2mat_ryxz(yaw, pitch, roll).T @ self.R

    def horizontal_flip(self):
        self.R[0] *= -1


def euler2mat_ryxz(yaw, pitch, roll) -> np.ndarray:
    """transforms3d.euler.euler2mat(yaw, pitch, roll, 'ryxz') (transforms3d is not a dependency), float64 [3, 3].

    'ryxz' is the rotating-frame convention with axes y, x, z: the matrix is Ry(yaw) @ Rx(pitch) @ Rz(roll) with the
    right-handed elementary rotations Rx(a) = [[1, 0, 0], [0, c, -s], [0, s, c]], Ry(a) = [[c, 0, s], [0, 1, 0], [-s, 0, c]],
    Rz(a) = [[c, -s, 0], [s, c, 0], [0, 0, 1]].  Its entries are written as transforms3d's euler2mat writes them for this axis
    code (first axis z, no parity, no repetition, rotating frame: i, j, k = 2, 0, 1 with the first and last angle swapped),
    so roll alone gives exactly cos(roll) and sin(roll)."""
    si, sj, sk = math.sin(roll), math.sin(pitch), math.sin(yaw)
    ci, cj, ck = math.cos(roll), math.cos(pitch), math.cos(yaw)
    cc, cs, sc, ss = ci * ck, ci * sk, si * ck, si * sk
    m = np.eye(3)
    m[2, 2] = cj * ck
    m[2, 0] = sj * sc - cs
    m[2, 1] = sj * cc + ss
    m[0, 2] = cj * sk
    m[0, 0] = sj * ss + cc
    m[0, 1] = sj * cs - sc
    m[1, 2] = -sj
    m[1, 0] = cj * si
    m[1, 1] = cj * ci
    return m


def look_at_box(camera: Camera, box: Sequence[float], side: int = 256) -> Camera:
    """The virtual camera of a crop: reference cameralib.look_at_box (src/cameralib.py:337-358), step by step -- turn towards
    the box centre, undistort, square the pixels, zoom so that the box's longer side (measured between the two side midpoints,
    through the world) spans `side` pixels, centre the principal point.  This is the reference's stand-alone helper; the
    training loader's variant (data_loading.py:33-58: the norm of the side-point difference, a 1.05 box expansion for 3DHP,
    augmentation flags) is not what is restated here."""
    cam = camera.copy()
    box = np.asarray(box, np.float64)
    center_point = box[:2] + box[2:] / 2
    delta_x = np.array([box[2] / 2, 0])
    delta_y = np.array([0, box[3] / 2])
    if box[2] < box[3]:
        sidepoints = np.stack([center_point - delta_y, center_point + delta_y])
    else:
        sidepoints = np.stack([center_point - delta_x, center_point + delta_x])
    world_sidepoints = camera.image_to_world(sidepoints)
    cam.turn_towards(center_point)
    cam.undistort()
    cam.square_pixels()
    cam_sidepoints = cam.camera_to_image_undistorted(cam.world_to_camera(world_sidepoints))
    if box[2] < box[3]:
        crop_side = np.abs(cam_sidepoints[0, 1] - cam_sidepoints[1, 1])
    else:
        crop_side = np.abs(cam_sidepoints[0, 0] - cam_sidepoints[1, 0])
    cam.zoom(side / crop_side)
    cam.center_principal_point((side, side))
    return cam


class CropParams(NamedTuple):
    """Per-crop warp parameters (the fields of MetroCropWarp, include/metro_hip.h) and the rotations back."""
    mode: np.ndarray             # int32 [n]: _lib.METRO_WARP_HOMOGRAPHY | METRO_WARP_DISTORTED
    homography: np.ndarray       # float32 [n, 3, 3]
    partial: np.ndarray          # float64 [n, 3, 3]
    intrinsics: np.ndarray       # float32 [n, 3, 3] (the original camera's K)
    distortion: np.ndarray       # float32 [n, 5]
    rot_to_orig_cam: np.ndarray  # float32 [n, 3, 3]
    rot_to_world: np.ndarray     # float32 [n, 3, 3]


def _camera_of(cameras, f: int) -> Camera:
    if isinstance(cameras, Camera):
        return cameras
    return cameras[f]


def crop_params(cameras, boxes, frame_index, side: int = 256) -> CropParams:
    """Warp parameters of n crops.  `cameras`: None, one Camera for every frame, or a list with one Camera per frame.

    A camera with distortion_coeffs None takes the homography mode (reproject_image_fast, cameralib.py:406-412: K R of both
    cameras, solve, cast to float32); any coefficient array, even all zeros, takes the general mode (reproject_image case 2,
    :294-306: partial_homography = old.R inv(new.R) inv(new.K), float64), as the test at :272 sends it there.
    rot_to_orig_cam = orig.R virt.R^T and rot_to_world = virt.R^T (data_loading.py:110-111).
    cameras=None: the axis-aligned square crop of preprocess.box_homography, rotations I."""
    return _frame_params(cameras, boxes, frame_index, side)[0]


class PlacementParams(NamedTuple):
    """Per-crop placement records (the fields of MetroPlacement, include/metro_hip.h): the crop's virtual camera and the way
    back to its frame."""
    keypoint_mode: np.ndarray    # int32 [n]: _lib.METRO_WARP_HOMOGRAPHY | METRO_WARP_DISTORTED
    inv_intrinsics: np.ndarray   # float32 [n, 3, 3]: inv(virt.K) (data_loading.py:112); zero without a camera
    rot_to_orig_cam: np.ndarray  # float32 [n, 3, 3]
    rot_to_world: np.ndarray     # float32 [n, 3, 3]
    cam_loc: np.ndarray          # float32 [n, 3]: virt.t = orig.t
    homography: np.ndarray       # float32 [n, 3, 3]: crop pixel -> frame pixel (HOMOGRAPHY mode)
    intrinsics: np.ndarray       # float32 [n, 3, 3]: the original camera's K (DISTORTED mode)
    distortion: np.ndarray       # float32 [n, 5]


def placement_params(cameras, boxes, frame_index, side: int = 256) -> PlacementParams:
    """MetroPlacement records of n crops (`cameras` as for crop_params): inv_intrinsics = inv(virt.K) cast to float32,
    rot_to_orig_cam, rot_to_world and cam_loc = virt.t as the reference's loader returns them (data_loading.py:110-112, 119);
    the keypoint mode follows the warp mode (an undistorted camera or cameras=None: the crop's warp homography, which maps crop
    pixels to frame pixels; a camera with coefficients: its K and distortion for project_points).  cameras=None has no
    virtual camera: inv_intrinsics is zero (no metric placement) and the rotations are I."""
    return _frame_params(cameras, boxes, frame_index, side)[1]


def _frame_params(cameras, boxes, frame_index, side: int):
    """(CropParams, PlacementParams) of n crops, each virtual camera computed once."""
    return _frame_params_and_cameras(cameras, boxes, frame_index, side)[:2]


def _frame_params_and_cameras(cameras, boxes, frame_index, side: int):
    """(CropParams, PlacementParams, the look_at_box camera of every crop (None without cameras))."""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
    n = len(boxes)
    fi = np.asarray(frame_index, np.int64).reshape(n)
    p = CropParams(np.zeros(n, np.int32), np.zeros((n, 3, 3), np.float32), np.zeros((n, 3, 3)),
                   np.zeros((n, 3, 3), np.float32), np.zeros((n, 5), np.float32),
                   np.tile(np.eye(3, dtype=np.float32), (n, 1, 1)), np.tile(np.eye(3, dtype=np.float32), (n, 1, 1)))
    q = PlacementParams(p.mode, np.zeros((n, 3, 3), np.float32), p.rot_to_orig_cam, p.rot_to_world, np.zeros((n, 3), np.float32),
                        p.homography, p.intrinsics, p.distortion)
    virts = [None] * n
    for i, box in enumerate(boxes):
        if cameras is None:
            p.homography[i] = box_homography(box, side)
            continue
        orig = _camera_of(cameras, int(fi[i]))
        virt = virts[i] = look_at_box(orig, box, side)
        if orig.distortion_coeffs is None:
            old_matrix = orig.intrinsic_matrix @ orig.R                         # float32, as cameralib.py:410
            new_matrix = virt.intrinsic_matrix @ virt.R                         # float64 (square_pixels made K float64)
            p.homography[i] = np.linalg.solve(new_matrix.T, old_matrix.T).T.astype(np.float32)
        else:
            p.mode[i] = _lib.METRO_WARP_DISTORTED
            p.partial[i] = orig.R @ np.linalg.inv(virt.R) @ np.linalg.inv(virt.intrinsic_matrix)
            p.intrinsics[i] = orig.intrinsic_matrix
            p.distortion[i] = orig.distortion_coeffs
        p.rot_to_orig_cam[i] = (orig.R @ virt.R.T).astype(np.float32)
        p.rot_to_world[i] = virt.R.T.astype(np.float32)
        q.inv_intrinsics[i] = np.linalg.inv(virt.intrinsic_matrix).astype(np.float32)
        q.cam_loc[i] = virt.t
    return p, q, virts


def pack_crops(params: CropParams, frame_index) -> np.ndarray:
    """The MetroCropWarp records (include/metro_hip.h) of `params` as a byte array [n, 160]."""
    n = len(params.mode)
    rec = (_lib.MetroCropWarp * n)()
    k = params.intrinsics
    for i in range(n):
        r = rec[i]
        r.frame, r.mode = int(frame_index[i]), int(params.mode[i])
        r.partial[:] = params.partial[i].ravel().tolist()
        r.homography[:] = params.homography[i].ravel().tolist()
        r.intrinsics[:] = [float(v) for v in (k[i, 0, 0], k[i, 0, 1], k[i, 0, 2], k[i, 1, 0], k[i, 1, 1], k[i, 1, 2])]
        r.distortion[:] = params.distortion[i].tolist()
    return np.frombuffer(bytearray(rec), np.uint8).reshape(n, C.sizeof(_lib.MetroCropWarp))


def pack_placements(params: PlacementParams) -> np.ndarray:
    """The MetroPlacement records (include/metro_hip.h) of `params` as a byte array [n, 208]."""
    n = len(params.keypoint_mode)
    rec = (_lib.MetroPlacement * n)()
    k = params.intrinsics
    for i in range(n):
        r = rec[i]
        r.keypoint_mode = int(params.keypoint_mode[i])
        r.inv_intrinsics[:] = params.inv_intrinsics[i].ravel().tolist()
        r.rot_to_orig_cam[:] = params.rot_to_orig_cam[i].ravel().tolist()
        r.rot_to_world[:] = params.rot_to_world[i].ravel().tolist()
        r.cam_loc[:] = params.cam_loc[i].tolist()
        r.homography[:] = params.homography[i].ravel().tolist()
        r.intrinsics[:] = [float(v) for v in (k[i, 0, 0], k[i, 0, 1], k[i, 0, 2], k[i, 1, 0], k[i, 1, 1], k[i, 1, 2])]
        r.distortion[:] = params.distortion[i].tolist()
    return np.frombuffer(bytearray(rec), np.uint8).reshape(n, C.sizeof(_lib.MetroPlacement))


def _upload(a: np.ndarray, device: torch.device) -> torch.Tensor:
    """Host array -> device tensor without a host synchronisation (pinned staging, non-blocking copy)."""
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(device, non_blocking=True)


# ---- frames in other pixel formats: metro_warp_crops_frames_planes converts each tap as the warp reads it ----

PIXEL_FORMATS = {'rgb': _lib.METRO_PIX_RGB, 'bgr': _lib.METRO_PIX_BGR, 'nv12': _lib.METRO_PIX_NV12,
                 'i420': _lib.METRO_PIX_I420}
COLOR_MATRICES = {'bt601': _lib.METRO_YUV_BT601, 'bt709': _lib.METRO_YUV_BT709}
_LAYOUTS = {
    'rgb': 'a uint8 [H, W, 3] tensor or array',
    'bgr': 'a uint8 [H, W, 3] tensor or array',
    'nv12': 'a uint8 [H*3/2, W] tensor or array (Y rows, then interleaved UV rows) or a tuple (Y [H, W], UV [H/2, W/2, 2] '
            'or [H/2, W]), H and W even, rows of element stride 1',
    'i420': 'a contiguous uint8 [H*3/2, W] tensor or array (Y, then U and V at W/2 bytes per row) or a tuple (Y [H, W], '
            'U [H/2, W/2], V [H/2, W/2]) whose U and V share one row stride, H and W even, rows of element stride 1',
}


class _Planar(NamedTuple):
    """One frame for metro_warp_crops_frames_planes: its plane views (host or device) and the descriptor's fields."""
    planes: Tuple[torch.Tensor, ...]
    h: int
    w: int
    stride: Tuple[int, int]
    format: int
    matrix: int


class _FrameSet(NamedTuple):
    """Frames in a pixel format other than 'rgb' whose layouts are checked, as given (host or device data)."""
    items: list
    pixel_format: str
    color_matrix: str


def _frame_set(frames, pixel_format: str = 'rgb', color_matrix: str = 'bt601'):
    """Checks pixel_format and color_matrix and, for any format but 'rgb', the layout of every frame, before any device work.
    'rgb' frames come back as given, for the unchanged metro_warp_crops_frames_u8 path; the others as a _FrameSet.
    A YUV frame is one tensor / array (2-D) or a tuple of its planes; a list holds many frames."""
    if isinstance(frames, _FrameSet):
        return frames
    if pixel_format not in PIXEL_FORMATS:
        raise ValueError(f"pixel_format must be 'rgb', 'bgr', 'nv12' or 'i420', got {pixel_format!r}")
    if color_matrix not in COLOR_MATRICES:
        raise ValueError(f"color_matrix must be 'bt601' or 'bt709', got {color_matrix!r}")
    if pixel_format in ('rgb', 'bgr') and color_matrix != 'bt601':
        raise ValueError(f"color_matrix={color_matrix!r} applies to 'nv12' and 'i420' frames, not to {pixel_format!r} ones")
    if pixel_format == 'rgb':
        return frames
    if pixel_format == 'bgr':
        single = isinstance(frames, (torch.Tensor, np.ndarray)) and frames.ndim == 3
    else:
        single = isinstance(frames, (torch.Tensor, np.ndarray, tuple))
    items = [frames] if single else list(frames)
    if not items:
        raise ValueError('no frames')
    if len(items) > _lib.METRO_MAX_FRAMES:
        raise ValueError(f'{len(items)} frames: at most {_lib.METRO_MAX_FRAMES} per call')
    for k, f in enumerate(items):
        _planar(k, f, pixel_format, color_matrix)
    return _FrameSet(items, pixel_format, color_matrix)


def _planar(k: int, f, pixel_format: str, color_matrix: str) -> _Planar:
    """The plane views and descriptor fields of frame k (metadata only: no copy, no device work); ValueError on a bad layout."""
    def bad(what):
        return ValueError(f'frame {k}: {what}; pixel_format={pixel_format!r} takes {_LAYOUTS[pixel_format]}')

    def plane(t, name, ndim):
        t = torch.from_numpy(t) if isinstance(t, np.ndarray) else t
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != ndim:
            raise bad(f'{name} is {getattr(t, "dtype", type(t))} {tuple(getattr(t, "shape", ()))}')
        if pixel_format != 'bgr' and (t.stride(-1) != 1 or (ndim >= 2 and t.stride(0) < t.shape[1] * t.stride(1))):
            raise bad(f'{name} has strides {t.stride()}')
        return t

    def even(h, w):
        if h % 2 or w % 2:
            raise bad(f'{h} x {w} pixels (4:2:0 frames have an even height and width)')

    fmt, matrix = PIXEL_FORMATS[pixel_format], COLOR_MATRICES[color_matrix]
    if pixel_format == 'bgr':
        t = plane(f, 'the frame', 3)
        if t.shape[2] != 3:
            raise bad(f'the frame is {tuple(t.shape)}')
        return _Planar((t,), t.shape[0], t.shape[1], (t.stride(0), 0), fmt, matrix)
    n_planes = 2 if pixel_format == 'nv12' else 3
    if isinstance(f, tuple):
        if len(f) != n_planes:
            raise bad(f'a tuple of {len(f)} planes')
        y = plane(f[0], 'the Y plane', 2)
        h, w = y.shape
        even(h, w)
        if pixel_format == 'nv12':
            uv = f[1]
            uv = plane(uv, 'the UV plane', getattr(uv, 'ndim', 2))
            if tuple(uv.shape) not in ((h // 2, w // 2, 2), (h // 2, w)) or (uv.dim() == 3 and uv.stride(1) != 2):
                raise bad(f'the UV plane is {tuple(uv.shape)} with strides {uv.stride()} for a {h} x {w} Y plane')
            planes = (y, uv)
        else:
            u, v = plane(f[1], 'the U plane', 2), plane(f[2], 'the V plane', 2)
            if tuple(u.shape) != (h // 2, w // 2) or tuple(v.shape) != (h // 2, w // 2) or u.stride(0) != v.stride(0):
                raise bad(f'the U and V planes are {tuple(u.shape)} and {tuple(v.shape)} with row strides {u.stride(0)} and '
                          f'{v.stride(0)} for a {h} x {w} Y plane')
            planes = (y, u, v)
        if len({p.device for p in planes}) != 1:
            raise bad(f'the planes lie on {sorted({str(p.device) for p in planes})}')
        return _Planar(planes, h, w, (y.stride(0), planes[1].stride(0)), fmt, matrix)
    t = plane(f, 'the frame', 2)
    rows, w = t.shape
    if rows % 3:
        raise bad(f'the frame is {tuple(t.shape)}: {rows} rows are not H*3/2')
    h = rows * 2 // 3
    even(h, w)
    if pixel_format == 'nv12':
        return _Planar((t[:h], t[h:]), h, w, (t.stride(0), t.stride(0)), fmt, matrix)
    if not t.is_contiguous():
        raise bad(f'the frame has strides {t.stride()}')
    flat, q = t.reshape(-1), h * w // 4
    return _Planar((t[:h], flat[h * w:h * w + q].view(h // 2, w // 2), flat[h * w + q:].view(h // 2, w // 2)), h, w,
                   (w, w // 2), fmt, matrix)


def _device_frame_set(fs: _FrameSet, device: torch.device):
    """-> [_Planar] on the device: device frames as they are (a BGR one packed if it is not), host frames uploaded (pinned,
    non-blocking) at their own byte size."""
    def to_device(k, a):
        if isinstance(a, tuple):
            return tuple(to_device(k, p) for p in a)
        t = torch.from_numpy(a) if isinstance(a, np.ndarray) else a
        if not t.is_cuda:
            return _upload(t.numpy(), device)
        if t.device != device:
            raise ValueError(f'frame {k} is on {t.device}, the call runs on {device}')
        if fs.pixel_format == 'bgr' and (t.stride(2) != 1 or t.stride(1) != 3 or t.stride(0) < 3 * t.shape[1]):
            t = t.contiguous()
        return t
    return [_planar(k, to_device(k, f), fs.pixel_format, fs.color_matrix) for k, f in enumerate(fs.items)]


def _first_frame(frames):
    """The first frame (or plane) of `frames`, from which a call without device boxes takes its device."""
    f = frames.items if isinstance(frames, _FrameSet) else frames
    while isinstance(f, (list, tuple)) and f:
        f = f[0]
    return f if isinstance(f, (torch.Tensor, np.ndarray)) else None


def _device_frames(frames, device: torch.device):
    if isinstance(frames, _FrameSet):
        return _device_frame_set(frames, device)
    if isinstance(frames, (torch.Tensor, np.ndarray)) and frames.ndim == 3:
        frames = [frames]
    out = []
    for k, f in enumerate(frames):
        if isinstance(f, np.ndarray):
            f = torch.from_numpy(f)
        if not isinstance(f, torch.Tensor) or f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] != 3:
            raise ValueError(f'frame {k} must be a uint8 [H, W, 3] tensor or array, got '
                             f'{getattr(f, "dtype", type(f))} {tuple(getattr(f, "shape", ()))}')
        if f.is_cuda and f.device != device:
            raise ValueError(f'frame {k} is on {f.device}, the call runs on {device}')
        if not f.is_cuda:
            f = _upload(f.numpy(), device)
        if f.stride(2) != 1 or f.stride(1) != 3 or f.stride(0) < 3 * f.shape[1]:
            f = f.contiguous()
        out.append(f)
    if not out:
        raise ValueError('no frames')
    if len(out) > _lib.METRO_MAX_FRAMES:
        raise ValueError(f'{len(out)} frames: at most {_lib.METRO_MAX_FRAMES} per call')
    return out


def warp_frames(frames, params: CropParams, frame_index, side: int = 256, device: Optional[torch.device] = None,
                out: Optional[torch.Tensor] = None, pixel_format: str = 'rgb', color_matrix: str = 'bt601') -> torch.Tensor:
    """uint8 [H, W, 3] frames (a tensor or a list; host or device; sizes may differ) + per-crop parameters -> fp32 NHWC
    [n, side, side, 3] crops in [0, 1] on the device, in ONE launch on the current stream.
    pixel_format 'rgb' (metro_warp_crops_frames_u8), or 'bgr', 'nv12', 'i420' (metro_warp_crops_frames_planes: the bytes of
    'rgb' on the converted frame); color_matrix 'bt601' or 'bt709' for the YUV formats.  Frame layouts:
      'rgb', 'bgr'  uint8 [H, W, 3];
      'nv12'        uint8 [H*3/2, W] (Y rows then UV rows, as `ffmpeg -pix_fmt nv12 -f rawvideo` writes them; the row stride
                    is the tensor's), or a tuple (Y [H, W], UV [H/2, W/2, 2] or [H/2, W]), e.g. views into a pitched decoder
                    surface whose UV plane starts at an aligned offset;
      'i420'        contiguous uint8 [H*3/2, W] (Y, then U and V at W/2 bytes per row from offsets H W and H W 5/4), or a tuple
                    (Y [H, W], U [H/2, W/2], V [H/2, W/2]).
    A YUV frame is one tensor / array (2-D) or a tuple of planes; a list holds many frames.  H and W are even; rows have element
    stride 1; anything else raises ValueError naming the frame and the layout."""
    frames = _frame_set(frames, pixel_format, color_matrix)
    if device is None:
        first = _first_frame(frames)
        device = first.device if isinstance(first, torch.Tensor) and first.is_cuda else torch.device('cuda', torch.cuda.current_device())
    dev_frames = _device_frames(frames, device)
    n = len(params.mode)
    fi = np.asarray(frame_index, np.int64).reshape(n)
    if n and (fi.min() < 0 or fi.max() >= len(dev_frames)):
        raise ValueError(f'frame_index must lie in [0, {len(dev_frames)}), got [{fi.min()}, {fi.max()}]')
    if out is None:
        out = torch.empty((n, side, side, 3), dtype=torch.float32, device=device)
    if n == 0:
        return out
    _launch_warp(dev_frames, _upload(pack_crops(params, fi), device), n, side, out, device)
    return out


def _launch_warp(dev_frames, crops: torch.Tensor, n: int, side: int, out: torch.Tensor, device: torch.device) -> None:
    """One metro_warp_crops_frames_u8 launch ('rgb' frames: tensors) or one metro_warp_crops_frames_planes launch (_Planar
    frames) on the current stream: n MetroCropWarp records already on the device."""
    stream = torch.cuda.current_stream(device).cuda_stream
    if dev_frames and isinstance(dev_frames[0], _Planar):
        ptable = (_lib.MetroFramePlanes * len(dev_frames))()
        for k, f in enumerate(dev_frames):
            r = ptable[k]
            for i, p in enumerate(f.planes):
                r.plane[i] = p.data_ptr()
            r.h, r.w, r.format, r.matrix = f.h, f.w, f.format, f.matrix
            r.stride[0], r.stride[1] = f.stride
        check(_lib.load().metro_warp_crops_frames_planes(ptable, len(dev_frames), C.c_void_p(crops.data_ptr()), n, side,
                                                         C.c_void_p(out.data_ptr()), C.c_void_p(stream)),
              'metro_warp_crops_frames_planes')
        return
    table = (_lib.MetroFrame * len(dev_frames))()
    for k, f in enumerate(dev_frames):
        table[k].data, table[k].h, table[k].w, table[k].row_stride = f.data_ptr(), f.shape[0], f.shape[1], f.stride(0)
    check(_lib.load().metro_warp_crops_frames_u8(table, len(dev_frames), C.c_void_p(crops.data_ptr()), n, side,
                                                 C.c_void_p(out.data_ptr()), C.c_void_p(stream)), 'metro_warp_crops_frames_u8')


MAX_VIEWS = _lib.METRO_MAX_VIEWS
DEFAULT_ROLL_DEG = 20.0              # the reference's --rot-aug default (options.py:48-49)


class Views(NamedTuple):
    """A set of test-time views: view v is the look_at_box camera zoomed by zoom[v], rolled by roll_deg[v] about the optical
    axis and, if flip[v], mirrored horizontally -- in that order (data_loading.py:66-67, 77)."""
    roll_deg: np.ndarray         # float64 [V]
    zoom: np.ndarray             # float64 [V]
    flip: np.ndarray             # bool [V]


def view_set(views) -> Views:
    """`views` of estimate_pose_in_frames / locate_poses_in_frames -> Views.

    An int V (1 <= V <= 32) selects the default set: rolls linspace(-20, +20, V) degrees (the reference's --rot-aug range),
    zoom 1, a horizontal flip on the odd-indexed views; V = 1 is the identity view (roll 0, zoom 1, no flip).  E.g. V = 5:
    (-20, 1, False), (-10, 1, True), (0, 1, False), (10, 1, True), (20, 1, False).  Otherwise a sequence of 1 to 32
    (roll_deg, zoom, flip) triples: roll finite (degrees, positive turns the camera counter-clockwise about its optical axis,
    cameralib.Camera.rotate), zoom finite and > 0 (> 1 magnifies, about the principal point), flip a bool."""
    if isinstance(views, (bool, np.bool_)):
        raise ValueError(f'views must be an int (the default set) or (roll_deg, zoom, flip) triples, got {views!r}')
    if isinstance(views, (int, np.integer)):
        v = int(views)
        if not 1 <= v <= MAX_VIEWS:
            raise ValueError(f'views must lie in [1, {MAX_VIEWS}], got {v}')
        roll = np.linspace(-DEFAULT_ROLL_DEG, DEFAULT_ROLL_DEG, v) if v > 1 else np.zeros(1)
        return Views(roll, np.ones(v), np.arange(v) % 2 == 1)
    if isinstance(views, (str, bytes)) or not hasattr(views, '__len__'):
        raise ValueError(f'views must be an int (the default set) or (roll_deg, zoom, flip) triples, got {views!r}')
    if not 1 <= len(views) <= MAX_VIEWS:
        raise ValueError(f'views must hold 1 to {MAX_VIEWS} (roll_deg, zoom, flip) triples, got {len(views)}')
    roll, zoom, flip = np.zeros(len(views)), np.ones(len(views)), np.zeros(len(views), bool)
    for k, t in enumerate(views):
        if isinstance(t, (str, bytes)) or not hasattr(t, '__len__') or len(t) != 3:
            raise ValueError(f'view {k} must be a (roll_deg, zoom, flip) triple, got {t!r}')
        r, z, f = t
        if isinstance(r, (bool, np.bool_)) or not isinstance(r, (int, float, np.integer, np.floating)) or not math.isfinite(r):
            raise ValueError(f'view {k}: roll_deg must be a finite number, got {r!r}')
        if (isinstance(z, (bool, np.bool_)) or not isinstance(z, (int, float, np.integer, np.floating)) or not math.isfinite(z)
                or not z > 0):
            raise ValueError(f'view {k}: zoom must be a finite number > 0, got {z!r}')
        if not isinstance(f, (bool, np.bool_)):
            raise ValueError(f'view {k}: flip must be a bool, got {f!r}')
        roll[k], zoom[k], flip[k] = float(r), float(z), bool(f)
    return Views(roll, zoom, flip)


def _roll_rad(roll_deg: float) -> float:
    return float(roll_deg) * math.pi / 180


def _is_identity(vs: Views, v: int) -> bool:
    return vs.roll_deg[v] == 0 and vs.zoom[v] == 1 and not vs.flip[v]


def view_camera(camera: Camera, roll_deg: float, zoom: float, flip: bool) -> Camera:
    """A view of a look_at_box camera, as the reference's loader builds it under --test-aug (data_loading.py:60-68, 77):
    cam.zoom(zoom), cam.rotate(roll=roll), then cam.horizontal_flip() when flip."""
    cam = camera.copy()
    cam.zoom(zoom)
    cam.rotate(roll=_roll_rad(roll_deg))
    if flip:
        cam.horizontal_flip()
    return cam


def _square_crop_camera(side: int) -> Camera:
    """cameras=None: the square crop as a camera of principal point (side/2, side/2), unit focal length (roll, zoom and flip
    are image-plane similarities about that point whatever the focal length), R = I, K in float64 like look_at_box's."""
    cam = Camera(np.eye(3))
    cam.intrinsic_matrix = np.array([[1., 0, side / 2], [0, 1., side / 2], [0, 0, 1]])
    return cam


def view_params(cameras, boxes, frame_index, views, side: int = 256):
    """(CropParams, PlacementParams) of n * V crops, box-major (row i * V + v): the host restatement of metro_expand_views,
    _frame_params' formulas with each view camera (view_camera of the box's look_at_box camera) in place of the look_at_box
    one.  The identity view keeps the box's own records (its bits without views).  cameras=None: _square_crop_camera is the
    look_at_box camera and the square crop's homography its frame: homography = square's . K_base inv(K R), the rotations
    back R^T of the view, inv_intrinsics 0.  Tests use it as the reference of the device expansion; the product path does
    not call it."""
    vs = view_set(views)
    boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
    n, nv = len(boxes), len(vs.zoom)
    fi = np.asarray(frame_index, np.int64).reshape(n)
    p0, q0, virts = _frame_params_and_cameras(cameras, boxes, fi, side)
    rows = np.repeat(np.arange(n), nv)
    p = CropParams(*(np.array(a[rows]) for a in p0))
    q = PlacementParams(p.mode, q0.inv_intrinsics[rows], p.rot_to_orig_cam, p.rot_to_world, q0.cam_loc[rows], p.homography,
                        p.intrinsics, p.distortion)
    f32 = np.float32
    for i in range(n):
        base = _square_crop_camera(side) if cameras is None else virts[i]
        orig = None if cameras is None else _camera_of(cameras, int(fi[i]))
        for v in range(nv):
            if _is_identity(vs, v):
                continue
            r = i * nv + v
            view = view_camera(base, vs.roll_deg[v], vs.zoom[v], bool(vs.flip[v]))
            vk, vr = view.intrinsic_matrix, view.R
            if cameras is None:
                g = np.linalg.solve((vk @ vr).T, base.intrinsic_matrix.T).T
                p.homography[r] = (p0.homography[i].astype(np.float64) @ g).astype(f32)
                p.rot_to_orig_cam[r] = vr.T.astype(f32)
                p.rot_to_world[r] = vr.T.astype(f32)
                continue
            if orig.distortion_coeffs is None:
                old_matrix = orig.intrinsic_matrix @ orig.R                         # float32, as cameralib.py:410
                p.homography[r] = np.linalg.solve((vk @ vr).T, old_matrix.T).T.astype(f32)
            else:
                p.partial[r] = orig.R @ np.linalg.inv(vr) @ np.linalg.inv(vk)
            p.rot_to_orig_cam[r] = (orig.R @ vr.T).astype(f32)
            p.rot_to_world[r] = vr.T.astype(f32)
            q.inv_intrinsics[r] = np.linalg.inv(vk).astype(f32)
    return p, q


VIEW_BASE_DTYPE = np.dtype(_lib.MetroViewBase)


def pack_view_bases(cameras, boxes, frame_index, side: int = 256) -> np.ndarray:
    """The MetroViewBase records (include/metro_hip.h) of n boxes as a byte array [n, 576]: one look_at_box per box (through
    _frame_params, whose records are the identity view's), the rest filled column-wise, without a per-record ctypes loop."""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
    n = len(boxes)
    fi = np.asarray(frame_index, np.int64).reshape(n)
    p, q, virts = _frame_params_and_cameras(cameras, boxes, fi, side)
    rec = np.zeros(n, VIEW_BASE_DTYPE)
    rec['frame'] = fi
    rec['mode'] = p.mode
    rec['has_camera'] = int(cameras is not None)
    rec['partial'] = p.partial.reshape(n, 9)
    rec['homography'] = p.homography.reshape(n, 9)
    rec['inv_intrinsics'] = q.inv_intrinsics.reshape(n, 9)
    rec['rot_to_orig_cam'] = q.rot_to_orig_cam.reshape(n, 9)
    rec['rot_to_world'] = q.rot_to_world.reshape(n, 9)
    rec['cam_loc'] = q.cam_loc
    rec['intrinsics'] = p.intrinsics.reshape(n, 9)[:, :6]
    rec['distortion'] = p.distortion
    if cameras is not None and n:
        cams = [cameras] if isinstance(cameras, Camera) else list(cameras)
        slot = np.zeros(n, np.int64) if isinstance(cameras, Camera) else fi
        old = np.stack([(c.intrinsic_matrix @ c.R).astype(np.float64) for c in cams])   # float32 products, as cameralib.py:410
        rec['old_matrix'] = old.reshape(-1, 9)[slot]
        rec['orig_r'] = np.stack([c.R.astype(np.float64) for c in cams]).reshape(-1, 9)[slot]
        rec['virt_k'] = np.stack([np.asarray(v.intrinsic_matrix, np.float64) for v in virts]).reshape(n, 9)
        rec['virt_r'] = np.stack([np.asarray(v.R, np.float64) for v in virts]).reshape(n, 9)
    return rec.view(np.uint8).reshape(n, VIEW_BASE_DTYPE.itemsize)


def view_table(vs: Views):
    """The MetroView array of a view set: cos / sin of each roll computed here, once, in the arithmetic euler2mat_ryxz uses."""
    table = (_lib.MetroView * len(vs.zoom))()
    for v in range(len(vs.zoom)):
        a = _roll_rad(vs.roll_deg[v])
        table[v].cos_roll, table[v].sin_roll = math.cos(a), math.sin(a)
        table[v].zoom, table[v].flip = float(vs.zoom[v]), int(bool(vs.flip[v]))
    return table


def _expand_views(bases, vs: Views, side: int, device: torch.device):
    """One base-record upload (host records; device records, e.g. metro_look_at_boxes', are used in place) and one
    metro_expand_views launch -> (MetroCropWarp [n V, 160], MetroPlacement [n V, 208]) uint8 device tensors."""
    n, nv = len(bases), len(vs.zoom)
    d_bases = bases if isinstance(bases, torch.Tensor) else _upload(bases, device)
    crops = torch.empty((n * nv, C.sizeof(_lib.MetroCropWarp)), dtype=torch.uint8, device=device)
    places = torch.empty((n * nv, C.sizeof(_lib.MetroPlacement)), dtype=torch.uint8, device=device)
    stream = torch.cuda.current_stream(device).cuda_stream
    check(_lib.load().metro_expand_views(C.c_void_p(d_bases.data_ptr()), n, view_table(vs), nv, side,
                                         C.c_void_p(crops.data_ptr()), C.c_void_p(places.data_ptr()), C.c_void_p(stream)),
          'metro_expand_views')
    return crops, places


def _warp_views(frames, cameras, boxes, fi, vs: Views, side: int, device: torch.device):
    """Per-box host geometry, the expansion and ONE warp launch of the n V crops -> (crops [n V, side, side, 3], placement
    records [n V, 208])."""
    dev_frames = _device_frames(frames, device)
    n = len(boxes)
    if n and (fi.min() < 0 or fi.max() >= len(dev_frames)):
        raise ValueError(f'frame_index must lie in [0, {len(dev_frames)}), got [{fi.min()}, {fi.max()}]')
    crop_recs, places = _expand_views(pack_view_bases(cameras, boxes, fi, side), vs, side, device)
    crops = torch.empty((n * len(vs.zoom), side, side, 3), dtype=torch.float32, device=device)
    _launch_warp(dev_frames, crop_recs, len(crops), side, crops, device)
    return crops, places


# ---- device geometry: the MetroViewBase records of the boxes computed on the GPU (metro_look_at_boxes) ----

GEOMETRY = ('host', 'device', 'auto')
FRAME_CAMERA_DTYPE = np.dtype(_lib.MetroFrameCamera)


def _geometry_of(geometry, boxes) -> str:
    """`geometry` of estimate_pose_in_frames / locate_poses_in_frames -> 'host' or 'device' ('auto': 'device' for CUDA boxes)."""
    if not isinstance(geometry, str) or geometry not in GEOMETRY:
        raise ValueError(f"geometry must be 'host', 'device' or 'auto', got {geometry!r}")
    if geometry == 'auto':
        return 'device' if isinstance(boxes, torch.Tensor) and boxes.is_cuda else 'host'
    return geometry


def _host_array(a):
    """Host data as given (a torch tensor, on the device or not, is copied to a NumPy array)."""
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a


def pack_frame_cameras(cameras, n_frames: Optional[int] = None) -> np.ndarray:
    """The MetroFrameCamera table (include/metro_hip.h) of `cameras` as a structured array: one entry for a single Camera (every
    frame), else one per frame (the first n_frames of the list, which must hold that many).  Filled column-wise, per frame:
    K, R, t and the distortion coefficients in fp32, the world-up vector in fp64, and the two per-frame products the host takes
    with NumPy, inv(R) as Camera.camera_to_world uses it and K R as pack_view_bases stores it."""
    cams = [cameras] if isinstance(cameras, Camera) else list(cameras)
    if not isinstance(cameras, Camera) and n_frames is not None:
        if len(cams) < n_frames:
            raise ValueError(f'cameras: {len(cams)} Camera objects for {n_frames} frames (one Camera, or one per frame)')
        cams = cams[:n_frames]
    if not 1 <= len(cams) <= _lib.METRO_MAX_FRAMES:
        raise ValueError(f'cameras: {len(cams)} entries (1 to {_lib.METRO_MAX_FRAMES})')
    for k, c in enumerate(cams):
        if not isinstance(c, Camera):
            raise ValueError(f'cameras[{k}] must be a frames.Camera, got {type(c)}')
    rec = np.zeros(len(cams), FRAME_CAMERA_DTYPE)
    rec['intrinsics'] = np.stack([c.intrinsic_matrix for c in cams]).reshape(-1, 9)
    rec['r'] = np.stack([c.R for c in cams]).reshape(-1, 9)
    rec['r_inv'] = np.stack([np.linalg.inv(c.R) for c in cams]).reshape(-1, 9)
    rec['t'] = np.stack([c.t for c in cams])
    rec['has_distortion'] = [c.distortion_coeffs is not None for c in cams]
    rec['distortion'] = np.stack([np.zeros(5, np.float32) if c.distortion_coeffs is None else c.distortion_coeffs for c in cams])
    rec['world_up'] = np.stack([np.asarray(c.world_up, np.float64).reshape(3) for c in cams])
    rec['old_matrix'] = np.stack([(c.intrinsic_matrix @ c.R).astype(np.float64) for c in cams]).reshape(-1, 9)
    return rec


class _DeviceBoxes:
    """Boxes on the device for metro_look_at_boxes: fp64 [n, 4], and the frame indices either as host int64 [n] (checked
    against the frame count before any launch) or as a device int32 [n] tensor (checked by the kernel's status)."""
    __slots__ = ('boxes', 'host_fi', 'device_fi')

    def __init__(self, boxes: torch.Tensor, host_fi: Optional[np.ndarray], device_fi: Optional[torch.Tensor]):
        self.boxes, self.host_fi, self.device_fi = boxes, host_fi, device_fi

    def __len__(self) -> int:
        return int(self.boxes.shape[0])


def _device_boxes(boxes, frame_index, device: torch.device) -> _DeviceBoxes:
    """boxes (a float32 / float64 CUDA tensor [n, 4], or host data that is uploaded once) and frame_index (None, host data or a
    CUDA integer tensor) -> _DeviceBoxes, without a synchronisation."""
    if isinstance(boxes, torch.Tensor) and boxes.is_cuda:
        if boxes.device != device:
            raise ValueError(f'boxes are on {boxes.device}, the call runs on {device}')
        if boxes.dtype not in (torch.float32, torch.float64) or boxes.dim() != 2 or boxes.shape[1] != 4:
            raise ValueError(f'boxes must be a float32 or float64 [n, 4] (x, y, w, h) tensor, got {boxes.dtype} '
                             f'{tuple(boxes.shape)}')
        d_boxes = boxes.to(torch.float64).contiguous()
    else:
        b = np.asarray(_host_array(boxes), np.float64)
        if b.ndim != 2 or b.shape[1] != 4:
            raise ValueError(f'boxes must be [n, 4] (x, y, w, h), got {b.shape}')
        d_boxes = _upload(b, device)
    n = int(d_boxes.shape[0])
    if isinstance(frame_index, torch.Tensor) and frame_index.is_cuda:
        if frame_index.device != device:
            raise ValueError(f'frame_index is on {frame_index.device}, the call runs on {device}')
        if frame_index.is_floating_point() or frame_index.is_complex() or frame_index.dtype == torch.bool:
            raise ValueError(f'frame_index must hold integers, got {frame_index.dtype}')
        if frame_index.numel() != n:
            raise ValueError(f'frame_index must hold {n} values (one per box), got {frame_index.numel()}')
        fi = frame_index.reshape(n)
        if fi.dtype != torch.int32:         # out-of-range values stay out of range through the cast
            fi = fi.to(torch.int64).clamp(-1, _lib.METRO_MAX_FRAMES).to(torch.int32)
        return _DeviceBoxes(d_boxes, None, fi.contiguous())
    fi = np.zeros(n, np.int64) if frame_index is None else np.asarray(_host_array(frame_index), np.int64).reshape(n)
    return _DeviceBoxes(d_boxes, fi, None)


def _look_at_boxes(cameras, d_boxes: torch.Tensor, d_fi: torch.Tensor, n_frames: int, side: int, device: torch.device):
    """One camera-table upload (none for cameras=None) and one metro_look_at_boxes launch -> (MetroViewBase [n, 576] uint8,
    status int32 [1]: the number of frame indices outside [0, n_frames)) device tensors.  n >= 1."""
    n = int(d_boxes.shape[0])
    bases = torch.empty((n, VIEW_BASE_DTYPE.itemsize), dtype=torch.uint8, device=device)
    status = torch.empty(1, dtype=torch.int32, device=device)
    table, n_cameras = None, 0
    if cameras is not None:
        rec = pack_frame_cameras(cameras, n_frames)
        table, n_cameras = _upload(rec.view(np.uint8), device), len(rec)
    ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    stream = torch.cuda.current_stream(device).cuda_stream
    check(_lib.load().metro_look_at_boxes(ptr(d_boxes), ptr(d_fi), n, n_frames, ptr(table), n_cameras, side, ptr(bases),
                                          ptr(status), C.c_void_p(stream)), 'metro_look_at_boxes')
    return bases, status


def look_at_boxes(cameras, boxes, frame_index=None, side: int = 256, n_frames: Optional[int] = None,
                  device: Optional[torch.device] = None) -> torch.Tensor:
    """The device twin of pack_view_bases: the MetroViewBase records of n boxes computed by metro_look_at_boxes, as a uint8
    device tensor [n, 576].  boxes: a float32 / float64 CUDA tensor [n, 4] or host data; frame_index: None (frame 0), host
    data or a CUDA integer tensor; cameras: None, one Camera, or one Camera per frame.  n_frames (default: len(cameras) for
    a list, else METRO_MAX_FRAMES) bounds the frame indices; one outside [0, n_frames) raises ValueError (this reads the
    kernel's status: one synchronisation)."""
    if device is None:
        device = boxes.device if isinstance(boxes, torch.Tensor) and boxes.is_cuda else \
            torch.device('cuda', torch.cuda.current_device())
    if n_frames is None:
        n_frames = len(cameras) if isinstance(cameras, (list, tuple)) else _lib.METRO_MAX_FRAMES
    db = _device_boxes(boxes, frame_index, device)
    n = len(db)
    if n == 0:
        return torch.empty((0, VIEW_BASE_DTYPE.itemsize), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        bases, status = _look_at_boxes(cameras, db.boxes, _checked_device_fi(db, n_frames, device), n_frames, side, device)
        _raise_on_bad_frames(int(status.item()), n, n_frames)
    return bases


def _checked_device_fi(db: _DeviceBoxes, n_frames: int, device: torch.device) -> torch.Tensor:
    """The device frame indices of db; host indices are checked here, before any launch, and uploaded."""
    if db.device_fi is not None:
        return db.device_fi
    fi = db.host_fi
    if len(fi) and (fi.min() < 0 or fi.max() >= n_frames):
        raise ValueError(f'frame_index must lie in [0, {n_frames}), got [{fi.min()}, {fi.max()}]')
    return _upload(fi.astype(np.int32), device)


def _raise_on_bad_frames(n_out: int, n: int, n_frames: int) -> None:
    if n_out:
        raise ValueError(f'frame_index must lie in [0, {n_frames}): {n_out} of {n} device frame indices lie outside')


def _warp_device_boxes(frames, cameras, db: _DeviceBoxes, vs: Views, side: int, device: torch.device):
    """_warp_views with the geometry on the device: metro_look_at_boxes, the expansion and ONE warp launch, no per-box host
    work -> (crops [n V, side, side, 3], placement records [n V, 208], (status int32 [1], n_frames)).  The status is read by
    the caller after its synchronisation (_raise_on_bad_frames)."""
    dev_frames = _device_frames(frames, device)
    n_frames = len(dev_frames)
    bases, status = _look_at_boxes(cameras, db.boxes, _checked_device_fi(db, n_frames, device), n_frames, side, device)
    crop_recs, places = _expand_views(bases, vs, side, device)
    crops = torch.empty((len(db) * len(vs.zoom), side, side, 3), dtype=torch.float32, device=device)
    _launch_warp(dev_frames, crop_recs, len(crops), side, crops, device)
    return crops, places, (status, n_frames)


def _merge_views(poses, keypoints, z, places, mirror, n: int, nv: int, spread: bool):
    """One metro_merge_views launch -> (poses [n, J, 3], keypoints [n, J, 2] or None, z [n] or None, spread [n, J] or None)."""
    nj = poses.shape[1]
    dev = poses.device
    out = torch.empty((n, nj, 3), dtype=torch.float32, device=dev)
    kp = torch.empty((n, nj, 2), dtype=torch.float32, device=dev) if keypoints is not None else None
    zo = torch.empty(n, dtype=torch.float32, device=dev) if z is not None else None
    sp = torch.empty((n, nj), dtype=torch.float32, device=dev) if spread else None
    ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    check(_lib.load().metro_merge_views(ptr(poses), ptr(keypoints), ptr(z), ptr(places), ptr(mirror), n, nv, nj, ptr(out),
                                        ptr(kp), ptr(zo), ptr(sp), C.c_void_p(stream)), 'metro_merge_views')
    return out, kp, zo, sp


_ROT_TO_ORIG_CAM = _lib.MetroPlacement.rot_to_orig_cam.offset // 4      # float index of the field in a MetroPlacement
_ROT_TO_WORLD = _lib.MetroPlacement.rot_to_world.offset // 4


def estimate_pose_in_frames(frames, boxes, model_path, cameras=None, frame_index=None, coords: str = 'camera',
                            precision: Optional[str] = None, check_finite: Optional[bool] = None, views=None,
                            geometry: str = 'auto', pixel_format: str = 'rgb', color_matrix: str = 'bt601'):
    """uint8 frames + person boxes [n, 4] (x, y, w, h) -> (poses [n, Jout, 3] mm, joint_edges, joint_names) like estimate_pose.

    frames: a uint8 [H, W, 3] tensor / array or a list of them (host or device, sizes may differ, at most 64), or frames in
    `pixel_format` (below);
    frame_index [n]: the frame of each box (default: every box on frame 0); cameras: None (axis-aligned square crops, what
    preprocess.box_homography gives), one Camera for all frames, or one Camera per frame.
    The poses are root-relative, in `coords`:
      'crop'    the virtual camera of each crop: what estimate_pose returns for the crops;
      'camera'  the original camera (volumetric.py:204-205, 277-281: rotation by rot_to_orig_cam, mirrored joints when
                det <= 0);
      'world'   rotation by rot_to_world only (root-relative poses carry no translation; volumetric.py:206-208 adds cam_loc
                to absolute ones).
    One enqueue chain on the current stream of the local device: frame and parameter uploads (pinned, non-blocking), one warp
    launch, estimate_pose's forward in <= 256-crop chunks on its cached engine with its finite screen (its one stream
    synchronisation), then metro_to_orig_cam.  Runs on the local device only (estimate_pose's shard=False): sharding across
    ranks is not supported here.
    views: None (one crop per box, the path above) or test-time views (view_set: an int V for the default set, or
    (roll_deg, zoom, flip) triples): the host geometry stays per box, metro_expand_views derives the n V crop records on the
    device, one warp launch cuts them, estimate_pose runs on the n V crops, metro_to_orig_cam rotates each view back (mirroring
    flipped views' joints) and metro_merge_views averages the views of each box.  coords='crop' takes one view only (the views
    have different virtual cameras); views=1 returns the bits of views=None.
    geometry: where the per-box crop geometry is computed.  'host': look_at_box in NumPy per box (boxes are host data);
    'device': one metro_look_at_boxes launch writes the per-box records on the GPU (boxes a float32 / float64 CUDA tensor
    [n, 4], or host boxes uploaded once; frame_index host data or a CUDA integer tensor), then metro_expand_views with the
    identity view when views=None: no per-box host work and no synchronisation before the forward; the records agree with the
    host's to a few fp32 ulp (include/metro_hip.h).  'auto' (default): 'device' for CUDA boxes, else 'host'.  With device
    boxes the call runs on the boxes' device; a device frame index outside [0, n_frames) raises ValueError (read from the
    kernel's status after the call's synchronisation).
    pixel_format: 'rgb' (default), 'bgr', 'nv12' or 'i420', with color_matrix 'bt601' (default) or 'bt709' for the YUV
    formats; the layouts are warp_frames'.  Frames other than 'rgb' go through metro_warp_crops_frames_planes, which
    converts each tap as the warp reads it: the crops are byte for byte those of the RGB frame that OpenCV's integer
    cvtColor(COLOR_YUV2RGB_NV12 / _I420) rule gives (not ffmpeg's swscale, which rounds differently), with a black border;
    no RGB frame is written, and host frames upload at their own size (1.5 bytes per pixel for YUV)."""
    from metro_pose3d_amd.inference import _engine_for, _resolve_device, estimate_pose
    frames = _frame_set(frames, pixel_format, color_matrix)
    geo = _geometry_of(geometry, boxes)
    if coords not in ('crop', 'camera', 'world'):
        raise ValueError(f"coords must be 'crop', 'camera' or 'world', got {coords!r}")
    vs = None if views is None else view_set(views)
    if vs is not None and coords == 'crop' and len(vs.zoom) > 1:
        raise ValueError(f"coords='crop' takes one view: the {len(vs.zoom)} views have different virtual cameras")
    if precision is None:
        precision = os.environ.get('METRO_PRECISION', 'f16')
    first = _first_frame(frames)
    if geo == 'device':
        device = _geometry_device(boxes, first)
        db = _device_boxes(boxes, frame_index, device)
        if len(db):
            return _estimate_pose_views(frames, db, model_path, cameras, None, coords, precision, check_finite,
                                        vs if vs is not None else view_set(1), device)
        boxes, frame_index = np.zeros((0, 4)), None
    boxes = np.asarray(_host_array(boxes), np.float64)
    if boxes.ndim != 2 or boxes.shape[1] != 4:
        raise ValueError(f'boxes must be [n, 4] (x, y, w, h), got {boxes.shape}')
    n = len(boxes)
    fi = np.zeros(n, np.int64) if frame_index is None else np.asarray(_host_array(frame_index), np.int64).reshape(n)
    device = _resolve_device(first if isinstance(first, torch.Tensor) else torch.empty(0))
    if vs is not None and n:
        return _estimate_pose_views(frames, boxes, model_path, cameras, fi, coords, precision, check_finite, vs, device)
    with torch.cuda.device(device):
        side = _engine_for(model_path, precision, device, max(n, 1)).spec.proc_side
        params = crop_params(cameras, boxes, fi, side)
        crops = warp_frames(frames, params, fi, side, device=device)
        poses, edges, names = estimate_pose(crops, model_path, precision=precision, check_finite=check_finite, shard=False)
        if coords == 'crop' or n == 0:
            return poses, edges, names
        sk = _engine_for(model_path, precision, device, max(n, 1)).spec.skeleton
        rot = _upload((params.rot_to_orig_cam if coords == 'camera' else params.rot_to_world).reshape(n, 9), device)
        mirror = _upload(np.asarray(sk.out_mirror, np.int32), device)
        out = torch.empty_like(poses)
        stream = torch.cuda.current_stream(device).cuda_stream
        check(_lib.load().metro_to_orig_cam(C.c_void_p(poses.data_ptr()), C.c_void_p(rot.data_ptr()),
                                            C.c_void_p(mirror.data_ptr()), C.c_void_p(out.data_ptr()), n, sk.n_out,
                                            C.c_void_p(stream)), 'metro_to_orig_cam')
    return out, edges, names


def _geometry_device(boxes, first) -> torch.device:
    """The device of a call with device geometry: the boxes' for CUDA boxes, else the frames' (or the current one)."""
    from metro_pose3d_amd.inference import _resolve_device
    if isinstance(boxes, torch.Tensor) and boxes.is_cuda:
        return _resolve_device(boxes)
    return _resolve_device(first if isinstance(first, torch.Tensor) else torch.empty(0))


def _estimate_pose_views(frames, boxes, model_path, cameras, fi, coords, precision, check_finite, vs: Views, device):
    """boxes: host boxes with their frame indices fi, or _DeviceBoxes (fi None: the geometry runs on the device)."""
    from metro_pose3d_amd.inference import _engine_for, estimate_pose
    n, nv = len(boxes), len(vs.zoom)
    with torch.cuda.device(device):
        side = _engine_for(model_path, precision, device, n * nv).spec.proc_side
        if isinstance(boxes, _DeviceBoxes):
            crops, places, (status, n_frames) = _warp_device_boxes(frames, cameras, boxes, vs, side, device)
        else:
            crops, places = _warp_views(frames, cameras, boxes, fi, vs, side, device)
            status = None
        poses, edges, names = estimate_pose(crops, model_path, precision=precision, check_finite=check_finite, shard=False)
        if status is not None:            # after estimate_pose's synchronisation (its finite screen), or the call's one read
            _raise_on_bad_frames(int(status.item()), n, n_frames)
        if coords == 'crop':                                           # one view (checked by the caller)
            return poses, edges, names
        sk = _engine_for(model_path, precision, device, n * nv).spec.skeleton
        at = _ROT_TO_ORIG_CAM if coords == 'camera' else _ROT_TO_WORLD
        rot = places.view(torch.float32)[:, at:at + 9].contiguous()
        mirror = _upload(np.asarray(sk.out_mirror, np.int32), device)
        placed = torch.empty_like(poses)
        stream = torch.cuda.current_stream(device).cuda_stream
        check(_lib.load().metro_to_orig_cam(C.c_void_p(poses.data_ptr()), C.c_void_p(rot.data_ptr()),
                                            C.c_void_p(mirror.data_ptr()), C.c_void_p(placed.data_ptr()), n * nv, sk.n_out,
                                            C.c_void_p(stream)), 'metro_to_orig_cam')
        out = _merge_views(placed, None, None, places, mirror, n, nv, spread=False)[0]
    return out, edges, names


class FramePoses(NamedTuple):
    """What locate_poses_in_frames returns."""
    poses: torch.Tensor                  # float32 [n, Jout, 3] mm on the device, in the requested coords
    keypoints2d: torch.Tensor            # float32 [n, Jout, 2] frame pixels on the device (NaN: behind the original camera)
    z_offset: Optional[torch.Tensor]     # float32 [n] mm (absolute modes: the root's depth in the virtual camera), else None
    joint_edges: np.ndarray
    joint_names: np.ndarray


SCALE_RECOVERY = {'metro': _lib.METRO_SCALE_METRO, 'bone-lengths': _lib.METRO_SCALE_BONE_LENGTHS,
                  'true-root-depth': _lib.METRO_SCALE_TRUE_ROOT_DEPTH}
COORDS = {'crop': _lib.METRO_COORDS_CROP, 'camera': _lib.METRO_COORDS_CAMERA, 'world': _lib.METRO_COORDS_WORLD}


# Skeletons of the model files seen so far, keyed like inference._engine_for (absolute path, mtime): a frozen GraphDef has no
# spec entry and is decoded whole to learn it, which must happen once per file, not once per call.
MAX_CACHED_SKELETONS = 16
_SKELETONS: 'OrderedDict[Tuple[str, float], object]' = OrderedDict()


def _model_skeleton(model_path):
    """The skeleton of a model file, read once per (path, mtime): the .npz spec entry alone, or a .pb decoded whole."""
    from metro_pose3d_amd.modelfile import SPEC_KEY, load_model
    from metro_pose3d_amd.spec import ModelSpec
    path = os.path.abspath(model_path)
    key = (path, os.path.getmtime(path))
    sk = _SKELETONS.get(key)
    if sk is not None:
        _SKELETONS.move_to_end(key)
        return sk
    with open(path, 'rb') as f:
        is_zip = f.read(2) == b'PK'
    sk = None
    if is_zip:
        with np.load(path, allow_pickle=False) as z:
            if SPEC_KEY in z.files:
                sk = ModelSpec.from_json(bytes(z[SPEC_KEY]).decode()).skeleton
    if sk is None:
        sk = load_model(path)[0].skeleton
    _SKELETONS[key] = sk
    while len(_SKELETONS) > MAX_CACHED_SKELETONS:
        _SKELETONS.popitem(last=False)
    return sk


def _placement_targets(scale_recovery, cameras, n, n_edges, bone_lengths, root_depth):
    """Checks the scale-recovery arguments; returns (bone lengths float64 [E] or [n, E], per-pose flag, root depths float32 [n])."""
    if scale_recovery not in SCALE_RECOVERY:
        raise ValueError(f"scale_recovery must be 'metro', 'bone-lengths' or 'true-root-depth', got {scale_recovery!r}")
    if scale_recovery == 'metro':
        if bone_lengths is not None or root_depth is not None:
            raise ValueError("bone_lengths / root_depth go with scale_recovery='bone-lengths' / 'true-root-depth'")
        return None, 0, None
    if cameras is None:
        raise ValueError(f"scale_recovery={scale_recovery!r} places poses metrically and needs calibrated cameras (their intrinsics): "
                         "cameras=None has none (2D keypoints and root-relative poses: scale_recovery='metro')")
    if scale_recovery == 'bone-lengths':
        if root_depth is not None:
            raise ValueError("root_depth goes with scale_recovery='true-root-depth'")
        if bone_lengths is None:
            raise ValueError(f"scale_recovery='bone-lengths' needs bone_lengths in mm, [E] or [n, E] over the model's {n_edges} "
                             'head edges (spec.skeleton.head_edges); no default table ships with the package')
        b = np.asarray(bone_lengths, np.float64)
        if b.shape not in ((n_edges,), (n, n_edges)):
            raise ValueError(f'bone_lengths must be [{n_edges}] or [{n}, {n_edges}] (mm over spec.skeleton.head_edges), got {b.shape}')
        if not (np.isfinite(b).all() and (b > 0).all()):
            raise ValueError('bone_lengths must be finite and positive (mm)')
        return np.ascontiguousarray(b), int(b.ndim == 2), None
    if bone_lengths is not None:
        raise ValueError("bone_lengths go with scale_recovery='bone-lengths'")
    if root_depth is None:
        raise ValueError("scale_recovery='true-root-depth' needs root_depth [n] in mm")
    r = np.asarray(root_depth, np.float64)
    if r.shape != (n,):
        raise ValueError(f'root_depth must be [{n}] (mm, one per box), got {r.shape}')
    if not (np.isfinite(r).all() and (r > 0).all()):
        raise ValueError('root_depth must be finite and positive (mm)')
    return None, 0, r.astype(np.float32)


def locate_poses_in_frames(frames, boxes, model_path, cameras=None, frame_index=None, scale_recovery: str = 'bone-lengths',
                           bone_lengths=None, root_depth=None, coords: str = 'camera', precision: Optional[str] = None,
                           check_finite: Optional[bool] = None, views=None, return_spread: bool = False,
                           geometry: str = 'auto', pixel_format: str = 'rgb', color_matrix: str = 'bt601'):
    """uint8 frames + person boxes -> FramePoses(poses, keypoints2d, z_offset, joint_edges, joint_names): where each person is
    in 3D and where each joint lands in its frame's pixels.  frames, boxes, frame_index, cameras, precision and check_finite as
    for estimate_pose_in_frames.

    scale_recovery (the reference's --scale-recovery names, volumetric.py:171-201):
      'metro'            root-relative poses: the bits of estimate_pose_in_frames(..., coords=coords); z_offset None;
      'bone-lengths'     needs cameras and bone_lengths in mm, [E] or [n, E] over spec.skeleton.head_edges: rays through each
                         crop's virtual camera, the reference's Levenberg-Marquardt z offset (metro_backproject_bone_lengths'
                         arithmetic), back_project;
      'true-root-depth'  needs cameras and root_depth [n] in mm: the root's z in the crop's virtual camera (the reference's
                         coords3d_true[:, -1, 2]).
    coords: 'crop' (the virtual camera), 'camera' (the original one: to_orig_cam, volumetric.py:204-205, 277-281) or 'world'
    (to_orig_cam(x, rot_to_world) + cam_loc for absolute poses, :206-208; rotation only in 'metro' mode).
    keypoints2d: heatmap_to_image(coords01.xy) mapped into the frame (cameralib.reproject_image_points, cameralib.py:241-262):
    through the crop's warp homography (cameras=None or an undistorted camera), or through rot_to_orig_cam and the original
    camera's project_points (a camera with coefficients).  NaN where the ray points behind the original camera.
    One enqueue chain on the current stream of the local device: uploads, one warp launch, metro_forward_coords01 in <= 256-crop
    chunks with the finite screen folded on the device, one metro_place_poses launch, then the call's one stream
    synchronisation (the screen).  No default bone-length table ships: the reference's come from its training data.
    views: None (one crop per box) or test-time views as for estimate_pose_in_frames: n V crops through the same chain
    (bone lengths and root depths repeated per view), each view placed by metro_place_poses in `coords` (flipped views'
    joints mirrored), then metro_merge_views: poses and z offsets averaged over the views, keypoints over the views whose
    keypoint is finite (a flipped view contributes its mirror joint's), NaN if none.  views=1 returns the bits of
    views=None.  return_spread=True returns (FramePoses, spread [n, Jout]): per joint, the RMS 3D distance in mm of the
    views from their mean (zeros with one view), a cheap agreement score.
    geometry: 'host', 'device' or 'auto' as for estimate_pose_in_frames (device boxes: metro_look_at_boxes, then the views
    chain with the identity view when views=None; bone_lengths and root_depth stay host data); a device frame index outside
    [0, n_frames) raises ValueError, read together with the finite screen in the call's one synchronisation.
    pixel_format, color_matrix: as for estimate_pose_in_frames ('bgr', 'nv12', 'i420' frames converted per tap in the warp,
    OpenCV's integer YUV rule, black border)."""
    from metro_pose3d_amd.inference import _engine_for, _resolve_device
    frames = _frame_set(frames, pixel_format, color_matrix)
    geo = _geometry_of(geometry, boxes)
    if coords not in COORDS:
        raise ValueError(f"coords must be 'crop', 'camera' or 'world', got {coords!r}")
    vs = None if views is None else view_set(views)
    if vs is not None and coords == 'crop' and len(vs.zoom) > 1:
        raise ValueError(f"coords='crop' takes one view: the {len(vs.zoom)} views have different virtual cameras")
    if precision is None:
        precision = os.environ.get('METRO_PRECISION', 'f16')
    if check_finite is None:
        check_finite = os.environ.get('METRO_CHECK_FINITE', '1') != '0'
    first = _first_frame(frames)
    if geo == 'device':
        device = _geometry_device(boxes, first)
        db = _device_boxes(boxes, frame_index, device)
        n = len(db)
        if n:
            sk = _model_skeleton(model_path)
            targets, per_pose, root_z = _placement_targets(scale_recovery, cameras, n, len(sk.head_edges), bone_lengths,
                                                           root_depth)
            names = np.empty(sk.n_out, dtype=object)
            names[:] = sk.names_bytes()
            res = _locate_poses_views(frames, db, model_path, cameras, None, scale_recovery, targets, per_pose, root_z, coords,
                                      precision, check_finite, vs if vs is not None else view_set(1), sk, names, device)
            return res if return_spread else res[0]
        boxes, frame_index = np.zeros((0, 4)), None
    boxes = np.asarray(_host_array(boxes), np.float64)
    if boxes.ndim != 2 or boxes.shape[1] != 4:
        raise ValueError(f'boxes must be [n, 4] (x, y, w, h), got {boxes.shape}')
    n = len(boxes)
    fi = np.zeros(n, np.int64) if frame_index is None else np.asarray(_host_array(frame_index), np.int64).reshape(n)
    sk = _model_skeleton(model_path)
    targets, per_pose, root_z = _placement_targets(scale_recovery, cameras, n, len(sk.head_edges), bone_lengths, root_depth)
    device = _resolve_device(first if isinstance(first, torch.Tensor) else torch.empty(0))
    names = np.empty(sk.n_out, dtype=object)
    names[:] = sk.names_bytes()
    if vs is not None and n:
        res = _locate_poses_views(frames, boxes, model_path, cameras, fi, scale_recovery, targets, per_pose, root_z, coords,
                                  precision, check_finite, vs, sk, names, device)
        return res if return_spread else res[0]
    res = _locate_poses(frames, boxes, model_path, cameras, fi, scale_recovery, targets, per_pose, root_z, coords, precision,
                        check_finite, sk, names, device)
    if return_spread:
        return res, torch.zeros((n, sk.n_out), dtype=torch.float32, device=device)
    return res


def _locate_poses(frames, boxes, model_path, cameras, fi, scale_recovery, targets, per_pose, root_z, coords, precision,
                  check_finite, sk, names, device) -> FramePoses:
    from metro_pose3d_amd.inference import _engine_for
    n = len(boxes)
    with torch.cuda.device(device):
        eng = _engine_for(model_path, precision, device, max(n, 1))
        spec = eng.spec
        poses = torch.empty((n, sk.n_out, 3), dtype=torch.float32, device=device)
        keypoints = torch.empty((n, sk.n_out, 2), dtype=torch.float32, device=device)
        z_offset = torch.empty(n, dtype=torch.float32, device=device) if scale_recovery != 'metro' else None
        if n == 0:
            return FramePoses(poses, keypoints, z_offset, sk.edges_array(), names)
        side = spec.proc_side
        crop_p, place_p = _frame_params(cameras, boxes, fi, side)
        crops = warp_frames(frames, crop_p, fi, side, device=device)
        rel = torch.empty((n, sk.n_out, 3), dtype=torch.float32, device=device)
        coords01 = torch.empty((n, sk.n_head, 3), dtype=torch.float32, device=device)
        bad = None
        for i in range(0, n, eng.max_batch):
            k = min(eng.max_batch, n - i)
            eng.forward(crops[i:i + k], out=rel[i:i + k], coords01=coords01[i:i + k])
            if check_finite:       # folded on the device after every chunk: ONE synchronisation per call, below
                cnt = eng.status_words(k).ne(0).sum()
                bad = cnt if bad is None else bad + cnt
        recs = _upload(pack_placements(place_p), device)
        mirror = _upload(np.asarray(sk.out_mirror, np.int32), device)
        d_targets = _upload(targets, device) if targets is not None else None
        d_root = _upload(root_z, device) if root_z is not None else None
        d_edges = _upload(np.asarray(sk.head_edges, np.int32).reshape(-1, 2), device) if targets is not None else None
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
        stream = torch.cuda.current_stream(device).cuda_stream
        check(_lib.load().metro_place_poses(ptr(coords01), ptr(rel), ptr(recs), n, C.byref(eng.cspec), SCALE_RECOVERY[scale_recovery],
                                            ptr(d_targets), per_pose, ptr(d_root), ptr(d_edges), len(sk.head_edges),
                                            ptr(mirror), COORDS[coords], ptr(poses), ptr(keypoints), ptr(z_offset),
                                            C.c_void_p(stream)), 'metro_place_poses')
        n_bad = int(bad.item()) if bad is not None else 0              # the call's one stream synchronisation
        if n_bad:
            raise _lib.NonFiniteError(
                f'{spec.arch_name} stride {spec.stride} in precision {precision!r}: {n_bad} of {n} crops reached the '
                'soft-argmax with non-finite statistics' +
                (' (fp16 storage overflows at 65504: run this model with precision f32m or f64)' if precision == 'f16' else ''))
    return FramePoses(poses, keypoints, z_offset, sk.edges_array(), names)


def _locate_poses_views(frames, boxes, model_path, cameras, fi, scale_recovery, targets, per_pose, root_z, coords, precision,
                        check_finite, vs: Views, sk, names, device):
    """locate_poses_in_frames with views: -> (FramePoses, spread [n, Jout]).  boxes: host boxes with their frame indices fi,
    or _DeviceBoxes (fi None: the geometry runs on the device)."""
    from metro_pose3d_amd.inference import _engine_for
    n, nv = len(boxes), len(vs.zoom)
    m = n * nv
    if per_pose:                                    # per-box targets, repeated per view by index (box-major rows)
        targets = np.repeat(targets, nv, axis=0)
    if root_z is not None:
        root_z = np.repeat(root_z, nv)
    with torch.cuda.device(device):
        eng = _engine_for(model_path, precision, device, m)
        spec = eng.spec
        side = spec.proc_side
        if isinstance(boxes, _DeviceBoxes):
            crops, places, (status, n_frames) = _warp_device_boxes(frames, cameras, boxes, vs, side, device)
        else:
            crops, places = _warp_views(frames, cameras, boxes, fi, vs, side, device)
            status = None
        rel = torch.empty((m, sk.n_out, 3), dtype=torch.float32, device=device)
        coords01 = torch.empty((m, sk.n_head, 3), dtype=torch.float32, device=device)
        bad = None
        for i in range(0, m, eng.max_batch):
            k = min(eng.max_batch, m - i)
            eng.forward(crops[i:i + k], out=rel[i:i + k], coords01=coords01[i:i + k])
            if check_finite:       # folded on the device after every chunk: ONE synchronisation per call, below
                cnt = eng.status_words(k).ne(0).sum()
                bad = cnt if bad is None else bad + cnt
        poses_v = torch.empty((m, sk.n_out, 3), dtype=torch.float32, device=device)
        keypoints_v = torch.empty((m, sk.n_out, 2), dtype=torch.float32, device=device)
        z_v = torch.empty(m, dtype=torch.float32, device=device) if scale_recovery != 'metro' else None
        mirror = _upload(np.asarray(sk.out_mirror, np.int32), device)
        d_targets = _upload(targets, device) if targets is not None else None
        d_root = _upload(root_z, device) if root_z is not None else None
        d_edges = _upload(np.asarray(sk.head_edges, np.int32).reshape(-1, 2), device) if targets is not None else None
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
        stream = torch.cuda.current_stream(device).cuda_stream
        check(_lib.load().metro_place_poses(ptr(coords01), ptr(rel), ptr(places), m, C.byref(eng.cspec), SCALE_RECOVERY[scale_recovery],
                                            ptr(d_targets), per_pose, ptr(d_root), ptr(d_edges), len(sk.head_edges),
                                            ptr(mirror), COORDS[coords], ptr(poses_v), ptr(keypoints_v), ptr(z_v),
                                            C.c_void_p(stream)), 'metro_place_poses')
        poses, keypoints, z_offset, spread = _merge_views(poses_v, keypoints_v, z_v, places, mirror, n, nv, spread=True)
        if status is None:
            n_bad = int(bad.item()) if bad is not None else 0          # the call's one stream synchronisation
        else:                                # the screen and the frame-index status in the call's one synchronisation
            words = status[0].to(torch.int64) if bad is None else torch.stack([status[0].to(torch.int64), bad.reshape(())])
            words = words.reshape(-1).tolist()
            n_bad = words[1] if len(words) > 1 else 0
            _raise_on_bad_frames(words[0], n, n_frames)
        if n_bad:
            raise _lib.NonFiniteError(
                f'{spec.arch_name} stride {spec.stride} in precision {precision!r}: {n_bad} of {m} view crops reached the '
                'soft-argmax with non-finite statistics' +
                (' (fp16 storage overflows at 65504: run this model with precision f32m or f64)' if precision == 'f16' else ''))
    return FramePoses(poses, keypoints, z_offset, sk.edges_array(), names), spread
