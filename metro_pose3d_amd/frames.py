"""Pose estimation on full camera frames: person boxes and (optionally calibrated, lens-distorted) cameras in, poses out.

The reference's test path (src/data/data_loading.py:33-58, 107-111) builds a virtual camera per person box that turns towards
the box centre, drops the lens distortion, squares the pixels and zooms so the box fills the crop; `cameralib.reproject_image`
(src/cameralib.py:265-324) warps the uint8 frame into it; after the net `volumetric.to_orig_cam` (src/model/volumetric.py:
204-216, 277-281) rotates the poses back into the original camera or the world.  Here:

  Camera, undistort_points, look_at_box   host geometry, the reference's camera restated in its dtypes (camera.py)
  pixel_format, color_matrix              frames as decoders leave them, 'rgb' (the default), 'bgr', 'nv12', 'i420', converted
                                          per tap inside the warp (frame_formats.py)
  crop_params                             per-crop warp mode + matrices and the rotations back (data_loading.py:110-111)
  placement_params                        per-crop virtual camera (inverse K, rotations, camera centre) and the way back to the
                                          frame's pixels (MetroPlacement records)
  pack_crops, pack_placements,            the host restatement of the records the device writes: what tests and tools compare
  view_params, warp_frames                against, and one warp launch over host-packed records; not on the product path
  view_set, pack_view_bases               test-time augmentation (`views=`): V rolled / zoomed / flipped views per box
                                          (data_loading.py:60-68, 77-79), expanded on the device (metro_expand_views) from one
                                          record per box and fused per box after the placement (metro_merge_views)
  look_at_boxes, pack_frame_cameras       the per-box records on the device (metro_look_at_boxes, `geometry='device'`, the
                                          default for CUDA boxes): look_at_box and pack_view_bases restated per thread from a
                                          per-frame camera table, so boxes from a GPU detector stay on the GPU and the call does
                                          no per-box host work ('host' keeps the NumPy geometry and its bits)
  estimate_pose_in_frames                 root-relative poses: ONE chain on one device, enqueued on the current stream, for
                                          host boxes, device boxes and views (views=None is the identity view): per-box
                                          records, metro_expand_views, one warp launch, the forward, metro_to_orig_cam,
                                          metro_merge_views
  locate_poses_in_frames                  absolute poses (bone-lengths / true-root-depth scale recovery, volumetric.py:171-208)
                                          and 2D frame keypoints: the same chain with one metro_place_poses launch after the
                                          forward
  triangulate_poses_in_frames             world poses of persons seen by several calibrated cameras: the same chain up to the
                                          forward (with the heat-map moments for the covariance weights), then ONE
                                          metro_triangulate_joints launch that intersects, per person and joint, the rays of
                                          all the crops that show the person (person_groups: the CSR grouping of the crop
                                          rows); no bone lengths and no root depth needed.  Nothing in the reference (one
                                          camera per example)
  match_poses_in_frames                   the same without a person_index: one metro_view_affinity launch (how close the
                                          per-joint rays of every two boxes pass) and one metro_cluster_views launch
                                          (complete-linkage clustering in one workgroup, which writes the CSR grouping on the
                                          device) between the forward and metro_triangulate_joints.  Nothing in the reference
  track_poses_in_frames                   poses of tracked persons smoothed over the frames of a video:
                                          locate_poses_in_frames(return_uncertainty=True) unchanged, then ONE
                                          metro_smooth_tracks launch: per track and joint a constant-velocity Kalman filter
                                          and Rauch-Tung-Striebel pass over the track's boxes in time order, each weighted
                                          by its heat-map covariance (track_groups: the CSR grouping; new_track_state: the
                                          filter state carried from call to call).  Nothing in the reference (one image
                                          per example)
  follow_poses_in_frames                  the same without a track_index: ONE metro_associate_tracks launch between the
                                          forward and metro_smooth_tracks walks the boxes in time order over a table of
                                          track slots (greedy assignment on the filter's predicted poses, births, persistent
                                          ids) and writes the CSR grouping on the device (time_steps: the CSR of the time
                                          steps; new_track_table: the tracks carried from call to call).  Nothing in the
                                          reference
  follow_rig_poses_in_frames              follow_world_poses_in_frames (a calibrated rig's video followed in the world) in which
                                          a person only ONE camera sees keeps feeding its track: metro_person_steps_labels,
                                          metro_person_rays and metro_associate_tracks_rays cost its rays against the tracks
                                          and place each joint on its ray as a measurement tight across the ray, wide along it
  predict_boxes_in_frames, frame_sizes    the boxes of the NEXT frames from the track table, for the frames between a
                                          detector's key frames: ONE metro_predict_boxes call advances every live track to
                                          each frame's time with the filter's own prediction, projects its joints through
                                          the frame's calibrated camera and writes one box per (frame, track), compacted on
                                          the device and fused with whatever boxes a detector did give; the rows go into the
                                          calls above as they are.  Nothing in the reference
  locate_tracked_poses_in_frames          locate_poses_in_frames between those key frames with each person's own track as the
                                          prior of each crop's heat-maps (metro_plan_bind_track_prior: the forward writes the
                                          prior rows from the track table and the posterior behind them): plain and posterior
                                          poses from the same launches, the posterior covariance and, per joint, the
                                          log-evidence a tracker gates with.  Nothing in the reference
  Follower                                one followed stream: follow_poses_in_frames or follow_world_poses_in_frames with the
                                          keywords checked once, the assignment rule chosen ('greedy', or 'optimal':
                                          metro_associate_tracks_optimal) and the table of tracks kept between calls

Divergences from the reference, on purpose (camera.py and frame_formats.py list their own):
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
    device geometry takes one ~6 us launch for 64 boxes (profiles/device_geometry_probe.json).
"""
from __future__ import annotations

import ctypes as C
import math
import os
from collections import OrderedDict
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from metro_pose3d_amd import _lib
from metro_pose3d_amd._lib import check
from metro_pose3d_amd.camera import (UNDISTORT_ITERATIONS, Camera, _roll_rad, _square_crop_camera,  # noqa: F401 -- the public
                                     euler2mat_ryxz, look_at_box, undistort_points, view_camera)    # names of this module
from metro_pose3d_amd.frame_formats import (COLOR_MATRICES, PIXEL_FORMATS, _LAYOUTS, _FrameSet, _Planar,  # noqa: F401
                                            _device_frames, _first_frame, _frame_set, _planar, _upload)
from metro_pose3d_amd.preprocess import box_homography


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
    return _frame_params_and_cameras(cameras, boxes, frame_index, side)[0]


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
    return _frame_params_and_cameras(cameras, boxes, frame_index, side)[1]


def _frame_params_and_cameras(cameras, boxes, frame_index, side: int):
    """(CropParams, PlacementParams, the look_at_box camera of every crop (None without cameras)) of n crops, each virtual
    camera computed once."""
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


def _check_frame_index(fi: np.ndarray, n_frames: int) -> None:
    """Host frame indices against the frame count, before any launch."""
    if len(fi) and (fi.min() < 0 or fi.max() >= n_frames):
        raise ValueError(f'frame_index must lie in [0, {n_frames}), got [{fi.min()}, {fi.max()}]')


CROP_DTYPES = {'float32': torch.float32, 'uint8': torch.uint8}


def _crop_dtype(crop_dtype) -> torch.dtype:
    if crop_dtype not in CROP_DTYPES:
        raise ValueError(f"crop_dtype must be 'float32' or 'uint8', got {crop_dtype!r}")
    return CROP_DTYPES[crop_dtype]


def warp_frames(frames, params: CropParams, frame_index, side: int = 256, device: Optional[torch.device] = None,
                out: Optional[torch.Tensor] = None, pixel_format: str = 'rgb', color_matrix: str = 'bt601',
                crop_dtype: str = 'float32') -> torch.Tensor:
    """uint8 [H, W, 3] frames (a tensor or a list; host or device; sizes may differ) + per-crop parameters -> fp32 NHWC
    [n, side, side, 3] crops in [0, 1] on the device, in ONE launch on the current stream.
    crop_dtype 'uint8': the crops are the remapped bytes themselves (metro_warp_crops_frames_u8_to_u8 / _planes_to_u8), uint8
    [n, side, side, 3]: float32(byte) / 255 is the 'float32' crop bit for bit, and estimate_pose takes them as they are.
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
    dtype = _crop_dtype(crop_dtype)
    frames = _frame_set(frames, pixel_format, color_matrix)
    if device is None:
        first = _first_frame(frames)
        device = first.device if isinstance(first, torch.Tensor) and first.is_cuda else torch.device('cuda', torch.cuda.current_device())
    dev_frames = _device_frames(frames, device)
    n = len(params.mode)
    fi = np.asarray(frame_index, np.int64).reshape(n)
    _check_frame_index(fi, len(dev_frames))
    if out is None:
        out = torch.empty((n, side, side, 3), dtype=dtype, device=device)
    elif out.dtype != dtype:
        raise ValueError(f'out is {out.dtype}, crop_dtype is {crop_dtype!r}')
    if n == 0:
        return out
    _launch_warp(dev_frames, _upload(pack_crops(params, fi), device), n, side, out, device)
    return out


def _launch_warp(dev_frames, crops: torch.Tensor, n: int, side: int, out: torch.Tensor, device: torch.device) -> None:
    """One metro_warp_crops_frames_u8 launch ('rgb' frames: tensors) or one metro_warp_crops_frames_planes launch (_Planar
    frames) on the current stream: n MetroCropWarp records already on the device.  A uint8 `out` takes the entries that write
    the remapped byte (metro_warp_crops_frames_u8_to_u8, metro_warp_crops_frames_planes_to_u8)."""
    stream = torch.cuda.current_stream(device).cuda_stream
    lib, u8 = _lib.load(), out.dtype == torch.uint8
    if dev_frames and isinstance(dev_frames[0], _Planar):
        ptable = (_lib.MetroFramePlanes * len(dev_frames))()
        for k, f in enumerate(dev_frames):
            r = ptable[k]
            for i, p in enumerate(f.planes):
                r.plane[i] = p.data_ptr()
            r.h, r.w, r.format, r.matrix = f.h, f.w, f.format, f.matrix
            r.stride[0], r.stride[1] = f.stride
        entry = 'metro_warp_crops_frames_planes_to_u8' if u8 else 'metro_warp_crops_frames_planes'
        check(getattr(lib, entry)(ptable, len(dev_frames), C.c_void_p(crops.data_ptr()), n, side,
                                  C.c_void_p(out.data_ptr()), C.c_void_p(stream)), entry)
        return
    table = (_lib.MetroFrame * len(dev_frames))()
    for k, f in enumerate(dev_frames):
        table[k].data, table[k].h, table[k].w, table[k].row_stride = f.data_ptr(), f.shape[0], f.shape[1], f.stride(0)
    entry = 'metro_warp_crops_frames_u8_to_u8' if u8 else 'metro_warp_crops_frames_u8'
    check(getattr(lib, entry)(table, len(dev_frames), C.c_void_p(crops.data_ptr()), n, side,
                              C.c_void_p(out.data_ptr()), C.c_void_p(stream)), entry)


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


def _is_identity(vs: Views, v: int) -> bool:
    return vs.roll_deg[v] == 0 and vs.zoom[v] == 1 and not vs.flip[v]


def view_params(cameras, boxes, frame_index, views, side: int = 256):
    """(CropParams, PlacementParams) of n * V crops, box-major (row i * V + v): the host restatement of metro_expand_views,
    _frame_params_and_cameras' formulas with each view camera (view_camera of the box's look_at_box camera) in place of the look_at_box
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
    _frame_params_and_cameras, whose records are the identity view's), the rest filled column-wise, without a per-record ctypes loop."""
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
    against the frame count before any launch) or as a device int32 [n] tensor (checked by the kernel's status).
    frame_status: None until _warp_views launched metro_look_at_boxes on these boxes, then (status int32 [1], n_frames),
    which the call reads in its synchronisation (_synchronise)."""
    __slots__ = ('boxes', 'host_fi', 'device_fi', 'frame_status')

    def __init__(self, boxes: torch.Tensor, host_fi: Optional[np.ndarray], device_fi: Optional[torch.Tensor]):
        self.boxes, self.host_fi, self.device_fi, self.frame_status = boxes, host_fi, device_fi, None

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
    _check_frame_index(db.host_fi, n_frames)
    return _upload(db.host_fi.astype(np.int32), device)


def _raise_on_bad_frames(n_out: int, n: int, n_frames: int) -> None:
    if n_out:
        raise ValueError(f'frame_index must lie in [0, {n_frames}): {n_out} of {n} device frame indices lie outside')


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


def _warp_views(frames, cameras, boxes, fi, vs: Views, side: int, device: torch.device, crop_dtype: str = 'float32'):
    """The frames on the device, one MetroViewBase record per box (host boxes with their frame indices fi: pack_view_bases,
    NumPy per box; _DeviceBoxes, fi None: metro_look_at_boxes, no per-box host work), the expansion and ONE warp launch of the
    n V crops -> (crops [n V, side, side, 3], placement records [n V, 208]).  Host frame indices are checked here, before
    any launch; metro_look_at_boxes' check of device ones is left in boxes.frame_status.  No launch for n = 0.
    crop_dtype 'uint8': uint8 crops (the remapped bytes), which the forward reads as they are."""
    dtype = _crop_dtype(crop_dtype)
    dev_frames = _device_frames(frames, device)
    n, n_frames = len(boxes), len(dev_frames)
    if n == 0:
        return (torch.empty((0, side, side, 3), dtype=dtype, device=device),
                torch.empty((0, C.sizeof(_lib.MetroPlacement)), dtype=torch.uint8, device=device))
    if isinstance(boxes, _DeviceBoxes):
        bases, status = _look_at_boxes(cameras, boxes.boxes, _checked_device_fi(boxes, n_frames, device), n_frames, side, device)
        boxes.frame_status = (status, n_frames)
    else:
        _check_frame_index(fi, n_frames)
        bases = pack_view_bases(cameras, boxes, fi, side)
    crop_recs, places = _expand_views(bases, vs, side, device)
    crops = torch.empty((n * len(vs.zoom), side, side, 3), dtype=dtype, device=device)
    _launch_warp(dev_frames, crop_recs, len(crops), side, crops, device)
    return crops, places


def _synchronise(bad: Optional[torch.Tensor], boxes, also: Optional[torch.Tensor] = None):
    """The one read of a call, after everything is enqueued: the finite screen folded on the device (`bad`; None: not asked for)
    and, for _DeviceBoxes, their frame status in one transfer.  ValueError for a device frame index outside its range.  Host
    boxes and no screen: nothing to read, no synchronisation.
    also: one more device integer the caller needs on the host (the persons metro_cluster_views found), read in the same
    transfer.  -> (the number of non-finite crops, that integer or None)."""
    if also is None and not isinstance(boxes, _DeviceBoxes):
        return (int(bad.item()) if bad is not None else 0), None
    words = [t.reshape(-1)[:1].to(torch.int64) for t in (boxes.frame_status[0] if isinstance(boxes, _DeviceBoxes) else None, bad, also)
             if t is not None]
    words = torch.cat(words).tolist()
    if isinstance(boxes, _DeviceBoxes):
        _raise_on_bad_frames(words.pop(0), len(boxes), boxes.frame_status[1])
    n_bad = words.pop(0) if bad is not None else 0
    return n_bad, (words.pop(0) if also is not None else None)


class _Call(NamedTuple):
    """The arguments estimate_pose_in_frames and locate_poses_in_frames share, checked."""
    frames: object               # as _frame_set returns them
    boxes: object                # host boxes float64 [n, 4], or _DeviceBoxes (device geometry, n >= 1)
    fi: Optional[np.ndarray]     # int64 [n]: the frame of each host box; None with _DeviceBoxes, which hold their own
    vs: Views                    # views=None: the identity view
    precision: str
    check_finite: bool
    crop_dtype: str = 'float32'  # dtype of the crops between the warp and the forward: 'float32' | 'uint8'


def _checked_call(frames, boxes, frame_index, coords, views, geometry, precision, check_finite, pixel_format,
                  color_matrix, crop_dtype: str = 'float32') -> _Call:
    """Every check that needs neither the model file nor, for host boxes, a device; the environment's defaults."""
    _crop_dtype(crop_dtype)
    frames = _frame_set(frames, pixel_format, color_matrix)
    geo = _geometry_of(geometry, boxes)
    if coords not in COORDS:
        raise ValueError(f"coords must be 'crop', 'camera' or 'world', got {coords!r}")
    vs = view_set(1 if views is None else views)
    if coords == 'crop' and len(vs.zoom) > 1:
        raise ValueError(f"coords='crop' takes one view: the {len(vs.zoom)} views have different virtual cameras")
    if precision is None:
        precision = os.environ.get('METRO_PRECISION', 'f16')
    if check_finite is None:
        check_finite = os.environ.get('METRO_CHECK_FINITE', '1') != '0'
    if geo == 'device':
        db = _device_boxes(boxes, frame_index, _call_device(boxes, frames))
        if len(db):
            return _Call(frames, db, None, vs, precision, check_finite, crop_dtype)
        boxes, frame_index = np.zeros((0, 4)), None
    boxes = np.asarray(_host_array(boxes), np.float64)
    if boxes.ndim != 2 or boxes.shape[1] != 4:
        raise ValueError(f'boxes must be [n, 4] (x, y, w, h), got {boxes.shape}')
    n = len(boxes)
    fi = np.zeros(n, np.int64) if frame_index is None else np.asarray(_host_array(frame_index), np.int64).reshape(n)
    return _Call(frames, boxes, fi, vs, precision, check_finite, crop_dtype)


def _call_device(boxes, frames) -> torch.device:
    """The device of a call: the boxes' for CUDA boxes and _DeviceBoxes, else the first frame's (or the current one)."""
    from metro_pose3d_amd.inference import _resolve_device
    if isinstance(boxes, _DeviceBoxes):
        boxes = boxes.boxes
    if isinstance(boxes, torch.Tensor) and boxes.is_cuda:
        return _resolve_device(boxes)
    first = _first_frame(frames)
    return _resolve_device(first if isinstance(first, torch.Tensor) else torch.empty(0))


def estimate_pose_in_frames(frames, boxes, model_path, cameras=None, frame_index=None, coords: str = 'camera',
                            precision: Optional[str] = None, check_finite: Optional[bool] = None, views=None,
                            geometry: str = 'auto', pixel_format: str = 'rgb', color_matrix: str = 'bt601',
                            crop_dtype: str = 'float32', return_uncertainty: bool = False):
    """uint8 frames + person boxes [n, 4] (x, y, w, h) -> (poses [n, Jout, 3] mm, joint_edges, joint_names) like estimate_pose.

    return_uncertainty=True adds a fourth element, inference.PoseUncertainty(covariance [n, Jout, 3, 3] mm^2, peak [n, Jout]):
    the covariance of each joint's own heat-map (estimate_pose), rotated into `coords` as R Cov R^T with the crop's
    rot_to_orig_cam / rot_to_world (mirror joints swapped where det R <= 0, as for the poses) and averaged over the views,
    as are the peaks (one metro_place_covariances launch).  It stays in MeTRo's metric scale.

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
    One enqueue chain on the current stream of the local device, the same for every kind of call: frame uploads (pinned,
    non-blocking), one record per box, metro_expand_views (the n V crop and placement records, written on the device), one
    warp launch, estimate_pose's forward on the n V crops in <= 256-crop chunks on its cached engine with its finite screen (its
    one stream synchronisation), metro_to_orig_cam on each view (mirroring flipped views' joints), then metro_merge_views,
    which averages the views of each box.  Runs on the local device only (estimate_pose's shard=False): sharding across ranks
    is not supported here.
    views: None (one crop per box: the identity view, whose records metro_expand_views copies and whose merge is the view
    itself, so views=None and views=1 are one path and one answer) or test-time views (view_set: an int V for the default
    set, or (roll_deg, zoom, flip) triples).  coords='crop' takes one view only (the views have different virtual cameras)
    and returns the forward's poses as they are.
    geometry: where the per-box record is computed.  'host': look_at_box in NumPy per box (boxes are host data), one upload;
    'device': one metro_look_at_boxes launch writes the per-box records on the GPU (boxes a float32 / float64 CUDA tensor
    [n, 4], or host boxes uploaded once; frame_index host data or a CUDA integer tensor): no per-box host work and no
    synchronisation before the forward; the records agree with the host's to a few fp32 ulp (include/metro_hip.h).  'auto'
    (default): 'device' for CUDA boxes, else 'host'.  With device boxes the call runs on the boxes' device; a device frame
    index outside [0, n_frames) raises ValueError (read from the kernel's status after the call's synchronisation).
    pixel_format: 'rgb' (default), 'bgr', 'nv12' or 'i420', with color_matrix 'bt601' (default) or 'bt709' for the YUV
    formats; the layouts are warp_frames'.  Frames other than 'rgb' go through metro_warp_crops_frames_planes, which
    converts each tap as the warp reads it: the crops are byte for byte those of the RGB frame that OpenCV's integer
    cvtColor(COLOR_YUV2RGB_NV12 / _I420) rule gives (not ffmpeg's swscale, which rounds differently), with a black border;
    no RGB frame is written, and host frames upload at their own size (1.5 bytes per pixel for YUV).
    crop_dtype: what the warp hands the network.  'float32' (default): byte / 255 as fp32, 12 bytes per pixel.  'uint8': the
    remapped byte itself, 3 bytes per pixel, which the forward reads by the same rule (metro_forward_u8; the parity
    precisions expand it first): the same poses bit for bit."""
    call = _checked_call(frames, boxes, frame_index, coords, views, geometry, precision, check_finite, pixel_format,
                         color_matrix, crop_dtype)
    res = _estimate_pose_views(call, model_path, cameras, coords, return_uncertainty)
    return res if return_uncertainty else res[:3]


def _place_covariances(spec, cov01, peak, places, coords: str, n: int, nv: int):
    """One metro_place_covariances launch -> inference.PoseUncertainty of the n boxes (empty without a launch for n = 0)."""
    from metro_pose3d_amd.heads import place_covariances
    from metro_pose3d_amd.inference import PoseUncertainty
    if n == 0:
        n_out = spec.skeleton.n_out
        return PoseUncertainty(peak.new_empty((0, n_out, 3, 3)), peak.new_empty((0, n_out)))
    return PoseUncertainty(*place_covariances(cov01, peak, spec, coords, places.reshape(-1) if coords != 'crop' else None, nv))


def _estimate_pose_views(call: _Call, model_path, cameras, coords, uncertainty: bool = False):
    """-> (poses, joint_edges, joint_names, PoseUncertainty or None)."""
    from metro_pose3d_amd.inference import _engine_for, _estimate_pose
    n, nv = len(call.boxes), len(call.vs.zoom)
    device = _call_device(call.boxes, call.frames)
    with torch.cuda.device(device):
        spec = _engine_for(model_path, call.precision, device, max(n * nv, 1)).spec
        crops, places = _warp_views(call.frames, cameras, call.boxes, call.fi, call.vs, spec.proc_side, device, call.crop_dtype)
        poses, edges, names, mom = _estimate_pose(crops, model_path, call.precision, call.check_finite, False, None,
                                                  'head' if uncertainty else None)
        _synchronise(None, call.boxes)         # after estimate_pose's synchronisation (its finite screen), or the call's one
        unc = _place_covariances(spec, mom[0], mom[1], places, coords, n, nv) if uncertainty else None
        if coords == 'crop' or n == 0:         # one view (_checked_call)
            return poses, edges, names, unc
        sk = spec.skeleton
        at = _ROT_TO_ORIG_CAM if coords == 'camera' else _ROT_TO_WORLD
        rot = places.view(torch.float32)[:, at:at + 9].contiguous()
        mirror = _upload(np.asarray(sk.out_mirror, np.int32), device)
        placed = torch.empty_like(poses)
        stream = torch.cuda.current_stream(device).cuda_stream
        check(_lib.load().metro_to_orig_cam(C.c_void_p(poses.data_ptr()), C.c_void_p(rot.data_ptr()),
                                            C.c_void_p(mirror.data_ptr()), C.c_void_p(placed.data_ptr()), n * nv, sk.n_out,
                                            C.c_void_p(stream)), 'metro_to_orig_cam')
        out = _merge_views(placed, None, None, places, mirror, n, nv, spread=False)[0]
    return out, edges, names, unc


class FramePoses(NamedTuple):
    """What locate_poses_in_frames returns."""
    poses: torch.Tensor                  # float32 [n, Jout, 3] mm on the device, in the requested coords
    keypoints2d: torch.Tensor            # float32 [n, Jout, 2] frame pixels on the device (NaN: behind the original camera)
    z_offset: Optional[torch.Tensor]     # float32 [n] mm (absolute modes: the root's depth in the virtual camera), else None
    joint_edges: np.ndarray
    joint_names: np.ndarray
    covariance: Optional[torch.Tensor] = None   # return_uncertainty: float32 [n, Jout, 3, 3] mm^2 in the requested coords, else None
    peak: Optional[torch.Tensor] = None         # return_uncertainty: float32 [n, Jout] largest heat-map probability, else None


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


def _placement_targets(scale_recovery, cameras, n, n_edges, bone_lengths, root_depth, device=None):
    """Checks the scale-recovery arguments; returns (bone lengths float64 [E] or [n, E], per-pose flag, root depths float32 [n]).
    A torch tensor as bone_lengths is device data: float64 [n, E], contiguous, on `device`; it is returned as it is, unread."""
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
        if isinstance(bone_lengths, torch.Tensor):
            t = bone_lengths
            if (not t.is_cuda or t.dtype != torch.float64 or tuple(t.shape) != (n, n_edges) or not t.is_contiguous()
                    or (device is not None and t.device != device)):
                raise ValueError(f'a tensor as bone_lengths must be a contiguous float64 CUDA tensor [{n}, {n_edges}] on the '
                                 f"call's device (Follower.bone_lengths_for), got {t.dtype} {tuple(t.shape)} on {t.device}; host "
                                 'values go in as arrays')
            return t, 1, None
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
                           geometry: str = 'auto', pixel_format: str = 'rgb', color_matrix: str = 'bt601',
                           crop_dtype: str = 'float32', return_uncertainty: bool = False):
    """uint8 frames + person boxes -> FramePoses(poses, keypoints2d, z_offset, joint_edges, joint_names): where each person is
    in 3D and where each joint lands in its frame's pixels.  frames, boxes, frame_index, cameras, precision and check_finite as
    for estimate_pose_in_frames.

    scale_recovery (the reference's --scale-recovery names, volumetric.py:171-201):
      'metro'            root-relative poses: the bits of estimate_pose_in_frames(..., coords=coords); z_offset None;
      'bone-lengths'     needs cameras and bone_lengths in mm, [E] or [n, E] over spec.skeleton.head_edges: rays through each
                         crop's virtual camera, the reference's Levenberg-Marquardt z offset (metro_backproject_bone_lengths'
                         arithmetic), back_project.  bone_lengths may also be a float64 CUDA tensor [n, E], contiguous and on
                         the call's device (Follower.bone_lengths_for: each followed person's own learned skeleton): it goes to
                         metro_place_poses as it is, repeated per view on the device, and its values are NOT read on the host --
                         they must be finite and positive, which bone_lengths_for guarantees; any other tensor is a ValueError
                         before any launch.  Host arrays keep their path and their bits;
      'true-root-depth'  needs cameras and root_depth [n] in mm: the root's z in the crop's virtual camera (the reference's
                         coords3d_true[:, -1, 2]).
    coords: 'crop' (the virtual camera), 'camera' (the original one: to_orig_cam, volumetric.py:204-205, 277-281) or 'world'
    (to_orig_cam(x, rot_to_world) + cam_loc for absolute poses, :206-208; rotation only in 'metro' mode).
    keypoints2d: heatmap_to_image(coords01.xy) mapped into the frame (cameralib.reproject_image_points, cameralib.py:241-262):
    through the crop's warp homography (cameras=None or an undistorted camera), or through rot_to_orig_cam and the original
    camera's project_points (a camera with coefficients).  NaN where the ray points behind the original camera.
    One enqueue chain on the current stream of the local device, estimate_pose_in_frames' up to the warp: uploads, one record
    per box, metro_expand_views, one warp launch; then metro_forward_coords01 in <= 256-crop chunks with the finite screen
    folded on the device, one metro_place_poses launch, metro_merge_views, then the call's one stream synchronisation (the
    screen).  No default bone-length table ships: the reference's come from its training data.
    views: None (one crop per box: the identity view) or test-time views as for estimate_pose_in_frames: n V crops (bone
    lengths and root depths repeated per view), each view placed by metro_place_poses in `coords` (flipped views' joints
    mirrored), then metro_merge_views: poses and z offsets averaged over the views, keypoints over the views whose keypoint
    is finite (a view whose rot_to_orig_cam has det <= 0 contributes its mirror joint's), NaN if none.  Every call runs the
    merge, so a camera whose own R is improper (det R <= 0) has its keypoints swapped to the mirror joints with or without
    views, on host and on device boxes alike.  return_spread=True returns (FramePoses, spread [n, Jout]): per joint, the RMS
    3D distance in mm of the views from their mean (zeros with one view), a cheap agreement score.
    geometry: 'host', 'device' or 'auto' as for estimate_pose_in_frames (root_depth stays host data, bone_lengths unless given as
    a CUDA tensor); a device frame index outside [0, n_frames) raises ValueError, read together with the finite screen in the call's one
    synchronisation.
    pixel_format, color_matrix: as for estimate_pose_in_frames ('bgr', 'nv12', 'i420' frames converted per tap in the warp,
    OpenCV's integer YUV rule, black border); crop_dtype 'float32' | 'uint8' likewise (the same bits from a quarter of the
    crop bytes).
    return_uncertainty=True fills FramePoses.covariance [n, Jout, 3, 3] (mm^2) and .peak [n, Jout] (None otherwise): the
    covariance of each joint's own heat-map (its softmax over the S x S x D volume; estimate_pose) in the requested coords --
    R Cov R^T per view, mirror joints swapped where det R <= 0, views averaged; one metro_place_covariances launch -- and the
    heat-map's largest probability.  The covariance stays in MeTRo's metric scale (the linear part of heatmap_to_metric) under
    every scale_recovery: bone lengths and root depths move and rescale the pose, they are not applied to it."""
    call = _checked_call(frames, boxes, frame_index, coords, views, geometry, precision, check_finite, pixel_format,
                         color_matrix, crop_dtype)
    sk = _model_skeleton(model_path)
    on_device = isinstance(bone_lengths, torch.Tensor) and bone_lengths.is_cuda
    targets, per_pose, root_z = _placement_targets(scale_recovery, cameras, len(call.boxes), len(sk.head_edges), bone_lengths,
                                                   root_depth, _call_device(call.boxes, call.frames) if on_device else None)
    res = _locate_poses_views(call, model_path, cameras, scale_recovery, targets, per_pose, root_z, coords, sk, return_uncertainty)
    return res if return_spread else res[0]


def _forward_coords01(eng, crops: torch.Tensor, check_finite: bool, moments: bool = False):
    """metro_forward_coords01 in chunks of the engine's batch -> (root-relative poses [m, Jout, 3], coords01 [m, Jhead, 3],
    the number of crops with non-finite statistics as a device scalar, or None without check_finite: folded on the device
    after every chunk, read by the caller's one synchronisation); `moments`: a fourth element (cov01 [m, Jhead, 6], peak
    [m, Jhead]) from the same launches."""
    sk = eng.spec.skeleton
    m = len(crops)
    rel = torch.empty((m, sk.n_out, 3), dtype=torch.float32, device=crops.device)
    coords01 = torch.empty((m, sk.n_head, 3), dtype=torch.float32, device=crops.device)
    cov01 = torch.empty((m, sk.n_head, 6), dtype=torch.float32, device=crops.device) if moments else None
    peak = torch.empty((m, sk.n_head), dtype=torch.float32, device=crops.device) if moments else None
    bad = None
    for i in range(0, m, eng.max_batch):
        k = min(eng.max_batch, m - i)
        if moments:
            eng.forward(crops[i:i + k], out=rel[i:i + k], coords01=coords01[i:i + k], cov01=cov01[i:i + k], peak=peak[i:i + k])
        else:
            eng.forward(crops[i:i + k], out=rel[i:i + k], coords01=coords01[i:i + k])
        if check_finite:
            cnt = eng.status_words(k).ne(0).sum()
            bad = cnt if bad is None else bad + cnt
    return (rel, coords01, bad, (cov01, peak)) if moments else (rel, coords01, bad)


def _joint_names(sk) -> np.ndarray:
    return np.array(sk.names_bytes(), dtype=object)


def _place_poses(eng, coords01, rel, places, scale_recovery: str, coords: str, d_targets=None, per_pose: int = 0, root_z=None):
    """One metro_place_poses launch over the m crop rows the forward wrote -> (poses [m, Jout, 3], keypoints [m, Jout, 2], z offsets
    [m] or None in 'metro' mode, the mirror table on the device).  d_targets: bone lengths on the device; root_z: host float32 [m]."""
    sk, m, device = eng.spec.skeleton, len(coords01), coords01.device
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)
    poses_v, keypoints_v, z_v = f32(m, sk.n_out, 3), f32(m, sk.n_out, 2), f32(m) if scale_recovery != 'metro' else None
    mirror = _upload(np.asarray(sk.out_mirror, np.int32), device)
    d_root = _upload(root_z, device) if root_z is not None else None
    d_edges = _upload(np.asarray(sk.head_edges, np.int32).reshape(-1, 2), device) if d_targets is not None else None
    ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    stream = torch.cuda.current_stream(device).cuda_stream
    check(_lib.load().metro_place_poses(ptr(coords01), ptr(rel), ptr(places), m, C.byref(eng.cspec), SCALE_RECOVERY[scale_recovery],
                                        ptr(d_targets), per_pose, ptr(d_root), ptr(d_edges), len(sk.head_edges), ptr(mirror),
                                        COORDS[coords], ptr(poses_v), ptr(keypoints_v), ptr(z_v), C.c_void_p(stream)),
          'metro_place_poses')
    return poses_v, keypoints_v, z_v, mirror


def _forward_tracked(eng, crops: torch.Tensor, check_finite: bool, places, nv: int, state, slots, times, prior: dict):
    """_forward_coords01 with the track prior bound (Engine.forward_track_posterior) -> (rel, coords01, bad, post [m, Jout, 11],
    reason [m, Jout]); slots and times hold one value per box and are repeated per view here, on the device."""
    sk = eng.spec.skeleton
    m = len(crops)
    rel = torch.empty((m, sk.n_out, 3), dtype=torch.float32, device=crops.device)
    coords01 = torch.empty((m, sk.n_head, 3), dtype=torch.float32, device=crops.device)
    mirror = _upload(np.asarray(sk.out_mirror, np.int32), crops.device)
    if nv > 1:
        slots, times = slots.repeat_interleave(nv), times.repeat_interleave(nv)
    posts, reasons, bad = [], [], None
    for i in range(0, m, eng.max_batch):
        k = min(eng.max_batch, m - i)
        _, post, _, reason = eng.forward_track_posterior(crops[i:i + k], state, slots[i:i + k], times[i:i + k], places[i:i + k], mirror,
                                                         out=rel[i:i + k], coords01=coords01[i:i + k], **prior)
        posts.append(post)
        reasons.append(reason)
        if check_finite:
            cnt = eng.status_words(k).ne(0).sum()
            bad = cnt if bad is None else bad + cnt
    return rel, coords01, bad, torch.cat(posts), torch.cat(reasons)


def _view_edge_columns(vs: Views, sk) -> np.ndarray:
    """int64 [V, E]: the bone-length column view v reads for edge e -- e itself, or in a flipped view (which shows every joint
    where its mirror joint is) Skeleton.edge_mirror()[e], -1 keeping the column."""
    straight = np.arange(len(sk.edges), dtype=np.int64)
    mirror = np.asarray(sk.edge_mirror(), np.int64).reshape(-1)
    flipped = np.where(mirror >= 0, mirror, straight)
    return np.stack([flipped if f else straight for f in vs.flip]).reshape(len(vs.flip), len(straight))


def _view_bone_rows(lengths: torch.Tensor, vs: Views, sk) -> torch.Tensor:
    """Bone lengths float64 [n, E] on the device -> [n V, E], one row per view row (box-major), unread: repeated per view, a
    flipped view's columns gathered through _view_edge_columns -- the flips are host-known."""
    cols = _upload(_view_edge_columns(vs, sk), lengths.device)
    return lengths[:, cols].reshape(-1, lengths.shape[1]).contiguous()


def _forward_skeleton(eng, crops: torch.Tensor, check_finite: bool, vs: Views, lengths, k, radius, options: dict):
    """_forward_coords01 with the modes and the skeleton bound (Engine.forward_skeleton_modes) -> (rel, coords01, bad, coords01_sel
    [m, Jhead, 3], choice [m, Jout], prob [m, Jout, k], info [m, Jout, 2]); lengths float64 [n, E] on the device, one row per box."""
    sk = eng.spec.skeleton
    m = len(crops)
    rel = torch.empty((m, sk.n_out, 3), dtype=torch.float32, device=crops.device)
    coords01 = torch.empty((m, sk.n_head, 3), dtype=torch.float32, device=crops.device)
    rows = _view_bone_rows(lengths, vs, sk)
    parts, bad = [], None
    for i in range(0, m, eng.max_batch):
        c = min(eng.max_batch, m - i)
        parts.append(eng.forward_skeleton_modes(crops[i:i + c], rows[i:i + c], k, radius, out=rel[i:i + c], coords01=coords01[i:i + c],
                                                **options)[3:])
        if check_finite:
            cnt = eng.status_words(c).ne(0).sum()
            bad = cnt if bad is None else bad + cnt
    choice, prob, info, sel = (torch.cat(t) for t in zip(*parts))
    return rel, coords01, bad, sel, choice, prob, info


def _locate_poses_views(call: _Call, model_path, cameras, scale_recovery, targets, per_pose, root_z, coords, sk,
                        uncertainty: bool = False, tracked=None, skeleton=None):
    """-> (FramePoses, spread [n, Jout]); tracked (the table's state, a slot and a time per box on the device, the prior keywords):
    (TrackedFramePoses, spread of the plain poses) from the same chain with the track prior bound; skeleton (bone lengths [n, E]
    on the device, k, radius, the options): (SkeletonFramePoses, spread of the plain poses) with the modes and the skeleton bound."""
    from metro_pose3d_amd.inference import _engine_for
    n, nv = len(call.boxes), len(call.vs.zoom)
    m = n * nv
    device = _call_device(call.boxes, call.frames)
    names = _joint_names(sk)
    with torch.cuda.device(device):
        eng = _engine_for(model_path, call.precision, device, max(m, 1))
        if n == 0:
            f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)
            unc = (f32(0, sk.n_out, 3, 3), f32(0, sk.n_out)) if uncertainty else (None, None)
            empty = FramePoses(f32(0, sk.n_out, 3), f32(0, sk.n_out, 2), f32(0) if scale_recovery != 'metro' else None,
                               sk.edges_array(), names, *unc)
            if tracked is not None:
                nv0 = (0, nv, sk.n_out)
                empty = TrackedFramePoses(empty, empty, f32(0, sk.n_out, 3, 3), f32(*nv0), f32(*nv0),
                                          torch.zeros(nv0, dtype=torch.int32, device=device))
            if skeleton is not None:
                nv0 = (0, nv, sk.n_out)
                empty = SkeletonFramePoses(empty, empty, torch.zeros(nv0, dtype=torch.int32, device=device), f32(*nv0, skeleton[1]),
                                           f32(*nv0), f32(*nv0))
            return empty, torch.zeros((0, sk.n_out), dtype=torch.float32, device=device)
        crops, places = _warp_views(call.frames, cameras, call.boxes, call.fi, call.vs, eng.spec.proc_side, device, call.crop_dtype)
        if tracked is not None:
            rel, coords01, bad, post, reason = _forward_tracked(eng, crops, call.check_finite, places, nv, *tracked)
        elif skeleton is not None:
            rel, coords01, bad, sel, choice, prob, info = _forward_skeleton(eng, crops, call.check_finite, call.vs, *skeleton)
        else:
            rel, coords01, bad, *mom = _forward_coords01(eng, crops, call.check_finite, uncertainty)
        if isinstance(targets, torch.Tensor):           # device bone lengths: unread, repeated per view on the device
            d_targets = targets if nv == 1 else targets.repeat_interleave(nv, dim=0)
        else:
            if per_pose:                                # per-box targets, repeated per view by index (box-major rows)
                targets = np.repeat(targets, nv, axis=0)
            d_targets = _upload(targets, device) if targets is not None else None
        root_rows = np.repeat(root_z, nv) if root_z is not None else None
        poses_v, keypoints_v, z_v, mirror = _place_poses(eng, coords01, rel, places, scale_recovery, coords, d_targets, per_pose, root_rows)
        poses, keypoints, z_offset, spread = _merge_views(poses_v, keypoints_v, z_v, places, mirror, n, nv, spread=True)
        unc = tuple(_place_covariances(eng.spec, mom[0][0], mom[0][1], places, coords, n, nv)) if uncertainty else (None, None)
        if tracked is not None:
            plain = FramePoses(poses, keypoints, z_offset, sk.edges_array(), names)
            both = _tracked_frame_poses(eng, plain, post, reason, coords01, places, scale_recovery, coords, d_targets, per_pose,
                                        root_rows, n, nv)
        if skeleton is not None:
            plain = FramePoses(poses, keypoints, z_offset, sk.edges_array(), names)
            both = _skeleton_frame_poses(eng, plain, sel, choice, prob, info, places, scale_recovery, coords, d_targets, per_pose,
                                         root_rows, n, nv)
        _raise_on_non_finite(eng.spec, call.precision, _synchronise(bad, call.boxes)[0], m)     # the call's one stream synchronisation
    if tracked is not None or skeleton is not None:
        return both, spread
    return FramePoses(poses, keypoints, z_offset, sk.edges_array(), names, *unc), spread


def _raise_on_non_finite(spec, precision: str, n_bad: int, m: int) -> None:
    if n_bad:
        raise _lib.NonFiniteError(
            f'{spec.arch_name} stride {spec.stride} in precision {precision!r}: {n_bad} of {m} crops reached the '
            'soft-argmax with non-finite statistics' +
            (' (fp16 storage overflows at 65504: run this model with precision f32m or f64)' if precision == 'f16' else ''))


# ---- several calibrated cameras per person: triangulated world poses (metro_triangulate_joints) ----

class WorldPoses(NamedTuple):
    """What triangulate_poses_in_frames returns."""
    poses: torch.Tensor                  # float32 [P, Jout, 3] world mm on the device; NaN where a joint is undetermined
    n_rays: torch.Tensor                 # int32 [P, Jout]: the rays in the joint's final solve (usable rays if undetermined)
    residual: torch.Tensor               # float32 [P, Jout] mm: weighted RMS distance of the joint from its rays
    keypoints2d: torch.Tensor            # float32 [n, Jout, 2] frame pixels of every box, as locate_poses_in_frames gives them
    joint_edges: np.ndarray
    joint_names: np.ndarray


def person_groups(person_index, frame_index, n_views: int = 1) -> Tuple[np.ndarray, np.ndarray]:
    """The CSR grouping metro_triangulate_joints reads, built on the host: (rows int32 [R], starts int32 [P + 1]) with
    P = max(person_index) + 1, person p owning rows[starts[p]:starts[p+1]] -- the crop rows i * n_views + v (box-major) of
    its boxes i, boxes in their given order (a stable sort by person).  A person index no box carries, and a person whose
    boxes all lie on ONE frame (one camera: its rays share an optical centre and fix no depth), get an empty group."""
    pi = np.asarray(person_index, np.int64).reshape(-1)
    fi = np.asarray(frame_index, np.int64).reshape(-1)
    if len(pi) != len(fi):
        raise ValueError(f'person_index holds {len(pi)} values, frame_index {len(fi)}')
    if len(pi) and pi.min() < 0:
        raise ValueError(f'person_index must not be negative, got {pi.min()}')
    n_persons = int(pi.max()) + 1 if len(pi) else 0
    pairs = np.unique(np.stack([pi, fi], axis=1), axis=0) if len(pi) else np.zeros((0, 2), np.int64)
    n_frames_of = np.bincount(pairs[:, 0], minlength=n_persons)
    order = np.argsort(pi, kind='stable')
    order = order[n_frames_of[pi[order]] >= 2]
    counts = np.bincount(pi[order], minlength=n_persons) * int(n_views)
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    rows = (order[:, None] * int(n_views) + np.arange(int(n_views))[None, :]).reshape(-1).astype(np.int32)
    return rows, starts


def triangulate_poses_in_frames(frames, boxes, model_path, cameras, person_index, frame_index, weights: str = 'covariance',
                                min_angle_deg: float = 2.0, views=None, precision: Optional[str] = None,
                                check_finite: Optional[bool] = None, geometry: str = 'auto', pixel_format: str = 'rgb',
                                color_matrix: str = 'bt601', crop_dtype: str = 'float32') -> WorldPoses:
    """uint8 frames of several calibrated cameras + person boxes -> WorldPoses(poses [P, Jout, 3], n_rays, residual,
    keypoints2d [n, Jout, 2], joint_edges, joint_names): the absolute world pose of every person from two or more views of
    it, with neither bone lengths nor a root depth.  frames, boxes, precision, check_finite, views, geometry, pixel_format,
    color_matrix and crop_dtype as for locate_poses_in_frames.

    cameras: a list with one Camera per frame, each with its own R and t (and distortion coefficients or None);
    frame_index [n]: the frame (camera) of each box; person_index [n]: whom each box shows, P = max(person_index) + 1.  Both
    are host integers.  Every box gives one ray per joint (V rays with views=V) from its crop's undistorted virtual camera,
    d = rot_to_world . K^-1 . heatmap_to_image(coords01) from cam_loc; joint r of person p is the point nearest to the rays
    of p's boxes (flipped views contribute their mirror joint, as in metro_place_poses).
    weights 'uniform': every ray counts alike.  'covariance' (default): a second solve in which a ray counts by
    1 / (sigma^2 z^2), sigma^2 the variance of the joint's own heat-map (the forward's moments, return_uncertainty's
    statistic) in normalised image units and z the ray's depth at the uniform solution: a joint one camera sees badly
    (occluded, at the crop's edge) leans on the cameras that see it well.
    A joint is undetermined -- NaN pose and residual, n_rays the usable rays -- with fewer than two rays, or when its rays are
    within min_angle_deg (in (0, 90], default 2 degrees) of parallel: the determinant of the normalised system is below
    sin^2(min_angle) / 4.  A person whose boxes all lie on one frame has rays from one optical centre only and is not
    solved: NaN pose, n_rays 0.  residual is the weighted RMS distance of the joint from its rays in mm: large where the
    views disagree (a wrong person association, a bad calibration).
    One enqueue chain on the current stream of the local device, locate_poses_in_frames' up to the forward (which also writes
    the heat-map moments in 'covariance' mode, from the same launches), then one metro_triangulate_joints launch over all
    n V crop rows, the keypoints by metro_place_poses and metro_merge_views, and the call's one synchronisation (the finite
    screen; NonFiniteError).  No boxes: empty tensors, no launch.  ValueError before any launch for cameras=None or one Camera
    for several frames, a negative person index, index lengths other than the number of boxes, an unknown `weights`, and
    min_angle_deg outside (0, 90]."""
    from metro_pose3d_amd.heads import Triangulation
    triangulation = Triangulation.checked(weights, min_angle_deg)
    n_boxes, fi, pi = _box_frames(boxes, frame_index, person_index, 'person_index')
    if n_boxes and pi.min() < 0:
        raise ValueError(f'person_index must not be negative, got {pi.min()}')
    _check_rig(cameras, fi, n_boxes)
    call = _checked_call(frames, boxes, fi, 'world', views, geometry, precision, check_finite, pixel_format, color_matrix,
                         crop_dtype)
    if len(call.boxes) == 0:
        return _no_persons(_model_skeleton(model_path), _call_device(call.boxes, call.frames)).world
    return _finish_world(call, _enqueue_world(call, model_path, cameras, fi, triangulation, person_index=pi))[0]


class FusedPoses(NamedTuple):
    """What fuse_poses_in_frames returns."""
    world: WorldPoses                    # triangulate_poses_in_frames' own, bit for bit
    poses: torch.Tensor                  # float32 [P, Jout, 3] world mm: the mean of the fused distribution; NaN where no row was usable
    covariance: torch.Tensor             # float32 [P, Jout, 3, 3] mm^2: its central second moments
    peak: torch.Tensor                   # float32 [P, Jout]: the largest weight of a grid point
    agreement: torch.Tensor              # float32 [P, Jout] <= 0: near 0 when all cameras' peaks meet in one point
    n_rows: torch.Tensor                 # int32 [P, Jout]: the crop rows used
    edge: torch.Tensor                   # int32 [P, Jout]: 1 where the heaviest grid point lies on the cube's surface (cube too small)


def fuse_poses_in_frames(frames, boxes, model_path, cameras, person_index, frame_index, weights: str = 'covariance',
                         min_angle_deg: float = 2.0, views=None, precision: Optional[str] = None,
                         check_finite: Optional[bool] = None, geometry: str = 'auto', pixel_format: str = 'rgb',
                         color_matrix: str = 'bt601', crop_dtype: str = 'float32', grid: int = 16, extent_mm: float = 1200.0,
                         floor: float = 1e-6, near_mm: float = 100.0) -> FusedPoses:
    """triangulate_poses_in_frames that also fuses every person's heat-maps over its cameras -> FusedPoses(world, poses
    [P, Jout, 3], covariance [P, Jout, 3, 3], peak, agreement, n_rows, edge).  Parameters as triangulate_poses_in_frames, plus the
    fusion's: grid, extent_mm, floor, near_mm (heads.fusion_params, which says of their defaults that they are design choices).

    The triangulation reduces every crop to the mean of its heat-map before the cameras meet; the mean of a two-peaked joint (a
    left / right swap, a second person in the crop) lies between the peaks and bends that camera's ray, and covariance weights
    only dilute the error.  The fusion keeps the distributions: on a cube of grid^3 world points of side extent_mm around every
    triangulated joint, each crop row gives a point the bilinear value of the joint's xy marginal at the point's projection
    (at least `floor`; a flipped view gives its mirror joint's), and the product of the rows -- with views=V each counting 1 / V
    -- is normalised over the cube.  A wrong peak in one camera finds no partner in the others and vanishes from the product.
    `poses` is the mean of that distribution, `covariance` its second moments, `peak` its largest weight; `agreement` <= 0 is
    the log of how far the best point falls short of all cameras' highest cells meeting there; `edge` says the cube was too
    small.  With TWO cameras a wrong peak's ray still meets the other camera's ray and nothing resolves it: that is inherent.
    On clean heat-maps the triangulated point is the better one (the bilinear probabilities are a coarser model than the
    soft-argmax): `world` is triangulate_poses_in_frames' result bit for bit, and the fusion stands beside it.  A joint the
    triangulation leaves undetermined has no centre: NaN, n_rows 0.
    One enqueue chain, triangulate_poses_in_frames' with the heat-maps and the fusion bound to its forward (the marginal
    launches, the centres' triangulation and view_fusion follow it), and the call's one synchronisation.  A known redundancy: the
    joints are triangulated twice on the same inputs, once inside the bound forward for the centres (its n_rays and residual
    are not kept) and once by triangulate_poses_in_frames' own launch for `world` (19 us a call as measured); that keeps
    `world` bit for bit with no further buffer bound.  All crop rows share
    ONE forward: ValueError where n V boxes-times-views exceed it.  ValueError before any launch as for
    triangulate_poses_in_frames, and for a fusion keyword out of range."""
    from metro_pose3d_amd.heads import Triangulation, fusion_params
    fusion = fusion_params(grid, extent_mm, floor, near_mm)
    triangulation = Triangulation.checked(weights, min_angle_deg)
    n_boxes, fi, pi = _box_frames(boxes, frame_index, person_index, 'person_index')
    if n_boxes and pi.min() < 0:
        raise ValueError(f'person_index must not be negative, got {pi.min()}')
    _check_rig(cameras, fi, n_boxes)
    call = _checked_call(frames, boxes, fi, 'world', views, geometry, precision, check_finite, pixel_format, color_matrix,
                         crop_dtype)
    if len(call.boxes) == 0:
        sk, device = _model_skeleton(model_path), _call_device(call.boxes, call.frames)
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=device)
        return FusedPoses(_no_persons(sk, device).world, f32(0, sk.n_out, 3), f32(0, sk.n_out, 3, 3), f32(0, sk.n_out), f32(0, sk.n_out),
                          i32(0, sk.n_out), i32(0, sk.n_out))
    chain = _enqueue_world(call, model_path, cameras, fi, triangulation, person_index=pi, fusion=fusion)
    world = _finish_world(call, chain)[0]
    points, cov, stats, info, _ = chain.fused
    return FusedPoses(world, points, cov.view(cov.shape[0], cov.shape[1], 3, 3), stats[..., 0], stats[..., 1], info[..., 0], info[..., 1])


def _n_boxes(boxes) -> int:
    return int(boxes.shape[0]) if isinstance(boxes, torch.Tensor) else len(np.asarray(boxes, np.float64).reshape(-1, 4))


def _box_frames(boxes, frame_index, other_index=None, other: str = ''):
    """(the number of boxes, frame_index as int64 [n]: None is frame 0), before any launch; with a second host index per box
    (person_index, track_index; `other`: its name), that one as int64 [n] too."""
    n_boxes = _n_boxes(boxes)
    fi = np.zeros(n_boxes, np.int64) if frame_index is None else np.asarray(_host_array(frame_index), np.int64).reshape(-1)
    if other_index is None:
        if len(fi) != n_boxes:
            raise ValueError(f'frame_index must hold one value per box ({n_boxes}), got {len(fi)}')
        return n_boxes, fi
    oi = np.asarray(_host_array(other_index), np.int64).reshape(-1)
    if len(oi) != n_boxes or len(fi) != n_boxes:
        raise ValueError(f'{other} and frame_index must hold one value per box ({n_boxes}), got {len(oi)} and {len(fi)}')
    return n_boxes, fi, oi


def _check_rig(cameras, fi: np.ndarray, n_boxes: int) -> None:
    """Several cameras need one calibrated Camera per frame, and every box a frame that has one."""
    if cameras is None:
        raise ValueError('triangulation needs calibrated cameras, one Camera per frame (cameras=None has none)')
    if isinstance(cameras, Camera):
        if n_boxes and (fi != fi[0]).any():
            raise ValueError('one Camera for several frames: triangulation needs one Camera per frame, each with its own R and t')
    elif n_boxes and (fi.min() < 0 or fi.max() >= len(cameras)):
        raise ValueError(f'frame_index must lie in [0, {len(cameras)}) (one Camera per frame), got [{fi.min()}, {fi.max()}]')


class _WorldChain(NamedTuple):
    """What _enqueue_world left on the stream: the device tensors of the chain up to the triangulation, unsliced (the per-person
    ones over the upper bound of n persons when the persons were found on the device)."""
    eng: object
    n: int                               # boxes
    nv: int                              # views per box
    rel: torch.Tensor                    # the forward's root-relative poses [n V, Jout, 3]
    coords01: torch.Tensor
    cov01: Optional[torch.Tensor]        # the heat-map moments, weights 'covariance' only
    places: torch.Tensor                 # MetroPlacement records uint8 [n V, 208]
    rows: torch.Tensor                   # the persons' crop rows as a CSR,
    starts: torch.Tensor                 # from the host (person_groups) or from metro_cluster_views
    labels: Optional[torch.Tensor]       # metro_cluster_views' person of every box,
    cost: Optional[torch.Tensor]         # the affinity's cost and
    n_pairs: Optional[torch.Tensor]      # ray pairs, and
    n_persons: Optional[torch.Tensor]    # the number of persons found int32 [1]; all four None with a host person_index
    poses: torch.Tensor
    n_rays: torch.Tensor
    residual: torch.Tensor
    covariance: Optional[torch.Tensor]   # [P, Jout, 9] of every triangulated joint, if asked for
    bad: Optional[torch.Tensor]          # the finite screen folded on the device
    fused: Optional[tuple] = None        # with `fusion`: Engine.forward_view_fusion's (points, cov, stats, info, centres)


def _forward_fused(eng, crops: torch.Tensor, check_finite: bool, moments: bool, places, rows, starts, nv: int, triangulation, fusion):
    """_forward_coords01 as ONE forward with the heat-maps and the view fusion bound (Engine.forward_view_fusion) -> (rel,
    coords01, bad, (cov01, peak) or None, (points, cov, stats, info, centres))."""
    sk, m = eng.spec.skeleton, len(crops)
    if m > eng.max_batch:
        raise ValueError(f'{m} crop rows exceed the {eng.max_batch} of one forward: a person\'s rows must share one forward')
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=crops.device)
    mom = (f32(m, sk.n_head, 6), f32(m, sk.n_head)) if moments else (None, None)
    mirror = _upload(np.asarray(sk.out_mirror, np.int32), crops.device)
    rel, coords01, *fused = eng.forward_view_fusion(crops, places.reshape(m, -1), rows, starts, int(starts.numel()) - 1, mirror, fusion,
                                                    triangulation.weights, triangulation.min_angle_deg, n_views=nv, cov01=mom[0],
                                                    peak=mom[1])
    bad = eng.status_words(m).ne(0).sum() if check_finite else None
    return rel, coords01, bad, mom if moments else None, tuple(fused)


def _enqueue_world(call: _Call, model_path, cameras, fi: np.ndarray, triangulation, person_index=None, matching=None,
                   step_index=None, covariance: bool = False, fusion=None) -> _WorldChain:
    """The first half of the chain triangulate_poses_in_frames, match_poses_in_frames and the world follower share, for n >= 1
    boxes: warp, forward, the persons' crop rows and ONE triangulation launch, nothing read back.  The rows come from the host
    (person_index: person_groups, uploaded) or, with `matching` (heads.Matching), from metro_view_affinity and
    metro_cluster_views on the forward's outputs; the triangulation launch then runs over the upper bound of n persons.
    step_index (host int32 [n], with matching): the affinity is gated by time step.  covariance: the triangulation launch also
    writes the covariance of every joint.  fusion (heads.Fusion, with person_index): the forward is ONE call with the heat-maps
    and the view fusion bound, whose outputs ride in the record's `fused`; the triangulation launch stays as it is.  A caller
    enqueues what it adds on the record's tensors, then _finish_world."""
    from metro_pose3d_amd.heads import cluster_views, triangulate_joints, view_affinity_steps
    from metro_pose3d_amd.inference import _engine_for
    n, nv = len(call.boxes), len(call.vs.zoom)
    device = _call_device(call.boxes, call.frames)
    moments = triangulation.weights == 'covariance'
    labels = cost = n_pairs = n_persons = None
    with torch.cuda.device(device):
        eng = _engine_for(model_path, call.precision, device, n * nv)
        crops, places = _warp_views(call.frames, cameras, call.boxes, call.fi, call.vs, eng.spec.proc_side, device, call.crop_dtype)
        fused = None
        if fusion is not None and matching is not None:
            raise ValueError('the view fusion reads the persons\' rows in the forward: persons found on the device (matching) are out of scope')
        if matching is None:
            rows, starts = (_upload(a, device) for a in person_groups(person_index, fi, nv))
        if fusion is not None:                                 # the fusion reads the persons' rows in the forward: host rows only
            rel, coords01, bad, mom, fused = _forward_fused(eng, crops, call.check_finite, moments, places, rows, starts, nv, triangulation,
                                                            fusion)
            mom = [mom]
        else:
            rel, coords01, bad, *mom = _forward_coords01(eng, crops, call.check_finite, moments)
        cov01 = mom[0][0] if moments else None
        if matching is not None:
            cost, n_pairs = view_affinity_steps(coords01, cov01, places.reshape(-1), _upload(fi.astype(np.int32), device),
                                                None if step_index is None else _upload(np.asarray(step_index, np.int32), device),
                                                eng.spec, nv, *triangulation, matching.clip_mm, matching.min_joints)
            labels, n_persons, rows, starts = cluster_views(cost, matching.max_cost_mm, nv)
        poses, n_rays, residual, *cov = triangulate_joints(coords01, cov01, places.reshape(-1), rows, starts, eng.spec, *triangulation,
                                                           covariance)
    return _WorldChain(eng, n, nv, rel, coords01, cov01, places, rows, starts, labels, cost, n_pairs, n_persons, poses, n_rays,
                       residual, cov[0] if covariance else None, bad, fused)


def _finish_world(call: _Call, chain: _WorldChain):
    """The second half: the keypoints by metro_place_poses and metro_merge_views, then the call's one stream synchronisation (the
    finite screen, which also brings the number of persons found on the device) -> (WorldPoses sliced to the persons, their
    number: None with a host person_index, where nothing is sliced).  NonFiniteError from the screen."""
    sk = chain.eng.spec.skeleton
    with torch.cuda.device(chain.coords01.device):
        poses_v, keypoints_v, _, mirror = _place_poses(chain.eng, chain.coords01, chain.rel, chain.places, 'metro', 'world')
        keypoints = _merge_views(poses_v, keypoints_v, None, chain.places, mirror, chain.n, chain.nv, spread=False)[1]
        n_bad, count = _synchronise(chain.bad, call.boxes, chain.n_persons)
        _raise_on_non_finite(chain.eng.spec, call.precision, n_bad, chain.n * chain.nv)
    return WorldPoses(chain.poses[:count], chain.n_rays[:count], chain.residual[:count], keypoints, sk.edges_array(),
                      _joint_names(sk)), count


def _no_persons(sk, device) -> 'MatchedPoses':
    """MatchedPoses, and in it the WorldPoses, of a call without boxes: empty tensors, no launch."""
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=device)
    return MatchedPoses(i32(0), f32(0, 0), i32(0, 0), WorldPoses(f32(0, sk.n_out, 3), i32(0, sk.n_out), f32(0, sk.n_out), f32(0, sk.n_out, 2),
                                                                 sk.edges_array(), _joint_names(sk)))


def _check_min_joints(min_joints, sk) -> None:
    if min_joints is not None and min_joints > sk.n_out:
        raise ValueError(f'min_joints must be at most the {sk.n_out} output joints of the model, got {min_joints!r}')


# ---- the same, with the persons found on the device: cross-view association (metro_view_affinity, metro_cluster_views) ----

class MatchedPoses(NamedTuple):
    """What match_poses_in_frames returns."""
    person_index: torch.Tensor           # int32 [n] on the device: the person of every box, numbered by their lowest box
    cost: torch.Tensor                   # float32 [n, n] mm: RMS distance between the rays of every two boxes (+inf: no match)
    n_pairs: torch.Tensor                # int32 [n, n]: the ray pairs behind each cost
    world: WorldPoses                    # triangulate_poses_in_frames' result for that person_index, P = the persons found


def match_poses_in_frames(frames, boxes, model_path, cameras, frame_index, max_cost_mm: float = 200.0, clip_mm: float = 500.0,
                          min_joints: Optional[int] = None, weights: str = 'covariance', min_angle_deg: float = 2.0, views=None,
                          precision: Optional[str] = None, check_finite: Optional[bool] = None, geometry: str = 'auto',
                          pixel_format: str = 'rgb', color_matrix: str = 'bt601', crop_dtype: str = 'float32') -> MatchedPoses:
    """triangulate_poses_in_frames without a person_index: which boxes show the same person is decided on the device, from the
    forward's own outputs, between the forward and the triangulation launch -> MatchedPoses(person_index int32 [n], cost
    [n, n], n_pairs [n, n], world: WorldPoses with one row per person found).  Every other argument as there; a person
    detector's boxes per camera, in any order, are enough.  At most 128 boxes.

    Two boxes of different frames show the same person when their per-joint rays pass close to each other: cost[a][b] is the
    RMS distance in mm between the rays of the same joint (heads.view_affinity: ray pairs within min_angle_deg of parallel
    left out, each distance capped at clip_mm, a pair that meets behind a camera counted as clip_mm; weights 'covariance'
    weighs each pair by its heat-maps' variances, and the moments are not requested in 'uniform' mode).  A cost from fewer
    than min_joints joints (per view; None: half the output joints, rounded up) is +inf, as is that of two boxes on one
    frame.  The boxes are then clustered (heads.cluster_views): the closest two clusters merge while their cost is below
    max_cost_mm, the cost between clusters being the largest between their boxes (complete linkage), so every two boxes of
    a person agree and no person has two boxes of one camera.  Persons are numbered by their lowest box.  A person seen by
    one camera only is a person with NaN poses and n_rays 0, as in triangulate_poses_in_frames.  The merge order is greedy,
    not an optimal assignment across cameras.
    max_cost_mm = 200, clip_mm = 500 and the min_joints default are design choices, not measurements: 200 mm is below the
    distance between two persons standing next to each other and above what calibration and heat-map error amount to at a
    few metres; 500 mm keeps one wild joint from deciding a pair; half the joints keeps a cost from resting on a few.
    One enqueue chain: triangulate_poses_in_frames' own, with one metro_view_affinity and one metro_cluster_views launch
    between the forward and metro_triangulate_joints, which runs over n persons (the upper bound; the groups past the persons
    found are empty); the call's one synchronisation stays the finite screen, which also brings the number of persons.
    ValueError before any launch for cameras=None or one Camera for several frames, a frame_index out of range or not one
    per box, more than 128 boxes, max_cost_mm, clip_mm, min_angle_deg or min_joints out of range and an unknown `weights`."""
    from metro_pose3d_amd.heads import MATCH_MAX_BOXES, Matching, Triangulation
    triangulation = Triangulation.checked(weights, min_angle_deg)
    matching = Matching.checked(max_cost_mm, clip_mm, min_joints)
    n_boxes, fi = _box_frames(boxes, frame_index)
    if n_boxes > MATCH_MAX_BOXES:
        raise ValueError(f'{n_boxes} boxes: matching takes at most {MATCH_MAX_BOXES} per call')
    _check_rig(cameras, fi, n_boxes)
    call = _checked_call(frames, boxes, fi, 'world', views, geometry, precision, check_finite, pixel_format, color_matrix,
                         crop_dtype)
    sk = _model_skeleton(model_path)
    _check_min_joints(matching.min_joints, sk)
    if len(call.boxes) == 0:
        return _no_persons(sk, _call_device(call.boxes, call.frames))
    chain = _enqueue_world(call, model_path, cameras, fi, triangulation, matching=matching)
    return MatchedPoses(chain.labels, chain.cost, chain.n_pairs, _finish_world(call, chain)[0])


# ---- one camera over time: tracked poses smoothed by a Kalman filter / RTS pass (metro_smooth_tracks) ----

class TrackPoses(NamedTuple):
    """What track_poses_in_frames returns."""
    poses: torch.Tensor                  # float32 [n, Jout, 3] mm: the filtered / smoothed pose of every box (untracked boxes: raw.poses)
    velocity: torch.Tensor               # float32 [n, Jout, 3] mm/s (NaN for untracked boxes)
    covariance: torch.Tensor             # float32 [n, Jout, 3, 3] mm^2 of the position estimate (untracked boxes: their R)
    used: torch.Tensor                   # uint8 [n, Jout]: 1 where the box's measurement entered the update
    raw: FramePoses                      # locate_poses_in_frames(..., return_uncertainty=True) of the same call, untouched
    state: torch.Tensor                  # float64 [T, Jout, 28]: the filter state after this call (pass it to the next)
    joint_edges: np.ndarray
    joint_names: np.ndarray


def track_groups(track_index, timestamps) -> Tuple[np.ndarray, np.ndarray]:
    """The CSR grouping metro_smooth_tracks reads, built on the host: (rows int32 [R], starts int32 [T + 1]) with
    T = max(track_index) + 1, track t owning rows[starts[t]:starts[t+1]], its rows in time order (a stable sort by track,
    then time).  track_index -1 means untracked: the row is in no group.  ValueError for other negative indices, for
    lengths that differ, for non-finite times and for two rows of one track at the same time."""
    ti = np.asarray(track_index, np.int64).reshape(-1)
    ts = np.asarray(timestamps, np.float64).reshape(-1)
    if len(ti) != len(ts):
        raise ValueError(f'track_index holds {len(ti)} values, timestamps {len(ts)}')
    if len(ti) and ti.min() < -1:
        raise ValueError(f'track_index must be a track (>= 0) or -1 for untracked, got {ti.min()}')
    if not np.isfinite(ts).all():
        raise ValueError('timestamps must be finite (seconds)')
    n_tracks = int(ti.max()) + 1 if len(ti) else 0
    order = np.lexsort((ts, ti))                           # by track, then time; stable
    order = order[ti[order] >= 0]
    same = (ti[order][1:] == ti[order][:-1]) & (ts[order][1:] == ts[order][:-1])
    if same.any():
        k = int(np.flatnonzero(same)[0])
        raise ValueError(f'track {ti[order][k]} has two rows at the same time {ts[order][k]!r} ({order[k]} and {order[k + 1]})')
    starts = np.concatenate([[0], np.cumsum(np.bincount(ti[order], minlength=n_tracks))]).astype(np.int32)
    return order.astype(np.int32), starts


def new_track_state(n_tracks: int, n_joints_out: int, device) -> torch.Tensor:
    """A float64 [n_tracks, n_joints_out, 28] filter state with no prior (t_last = NaN) for track_poses_in_frames /
    heads.smooth_tracks: per track and joint x (6), the upper triangle of P (21), t_last."""
    state = torch.zeros((int(n_tracks), int(n_joints_out), 28), dtype=torch.float64, device=device)
    state[..., 27] = float('nan')
    return state


def _box_times(timestamps, fi: np.ndarray, n: int) -> np.ndarray:
    """timestamps -> one float64 per box: n values are read per box (boxes of one frame must then agree), any other length per
    frame through frame_index."""
    ts = np.asarray(_host_array(timestamps), np.float64).reshape(-1)
    if not np.isfinite(ts).all():
        raise ValueError('timestamps must be finite (seconds)')
    if len(ts) != n:
        if n and (fi.min() < 0 or fi.max() >= len(ts)):
            raise ValueError(f'timestamps must hold one value per box ({n}) or one per frame: {len(ts)} values do not cover '
                             f'frame_index [{fi.min()}, {fi.max()}]')
        ts = ts[fi]
    else:
        first = {}
        for f, t in zip(fi.tolist(), ts.tolist()):
            if first.setdefault(f, t) != t:
                raise ValueError(f'timestamps: boxes on frame {f} carry different times ({first[f]!r} and {t!r}); pass one value per '
                                 'box, equal within a frame, or one per frame')
    return ts


def track_poses_in_frames(frames, boxes, model_path, cameras, track_index, frame_index, timestamps, state=None,
                          mode: str = 'smooth', measurement: str = 'covariance', accel_psd: float = 4e6,
                          sigma_floor_mm: float = 1.0, cov_scale: float = 1.0, initial_speed_mm_s: float = 2000.0, gate=None,
                          scale_recovery: str = 'bone-lengths', bone_lengths=None, root_depth=None, coords: str = 'camera',
                          precision: Optional[str] = None, check_finite: Optional[bool] = None, views=None,
                          geometry: str = 'auto', pixel_format: str = 'rgb', color_matrix: str = 'bt601',
                          crop_dtype: str = 'float32') -> TrackPoses:
    """uint8 frames of a video + person boxes with a track each -> TrackPoses(poses, velocity, covariance, used, raw, state,
    joint_edges, joint_names): locate_poses_in_frames(..., return_uncertainty=True), untouched (`raw`), then one
    metro_smooth_tracks launch that runs, per track and joint, a constant-velocity Kalman filter over the track's boxes in
    time order and (mode 'smooth') the Rauch-Tung-Striebel backward pass.  frames, boxes, cameras, frame_index and every
    keyword from scale_recovery on are locate_poses_in_frames'.

    track_index [n]: the track of each box (host integers; -1: untracked, the box comes back as `raw` has it with NaN
    velocity and used 0); associating boxes with tracks is the caller's here (follow_poses_in_frames does it on the device).
    timestamps: seconds, one value per box, or one per frame looked up through frame_index (n values are read per box); host data.  Two boxes of one track at one time are a
    ValueError.
    Each box's pose is a measurement with noise R = cov_scale * raw.covariance + sigma_floor_mm^2 I (measurement
    'isotropic': sigma_floor_mm^2 I): a joint whose heat-map is wide in some direction counts for less in that direction.
    A non-finite pose, or an R that is not positive definite, is bridged by the motion model (used 0); so is a measurement
    whose squared Mahalanobis innovation exceeds `gate` (None: no gate).  mode 'filter' returns the causal estimates.
    accel_psd (mm^2/s^3, white-noise acceleration), sigma_floor_mm and initial_speed_mm_s are design choices, not
    measurements (heads.smooth_tracks).
    state: None (every track starts at its first usable box; a fresh state for max(track_index) + 1 tracks is returned) or
    the state a previous call returned (new_track_state for more tracks than this call names): tracks continue from it, and
    it is updated in place with the FILTER state at each track's last box, so a stream cut into 64-frame calls with
    mode='filter' gives what one long call gives.  In mode 'smooth' a call smooths within itself; its last box per track is
    the filtered value.
    keypoints2d stay raw.keypoints2d: 2D smoothing is not offered."""
    from metro_pose3d_amd.heads import TRACK_STATE_DOUBLES, Smoothing, _smooth_tracks
    kw = locals()                                           # the keywords by name, for those handed on to locate_poses_in_frames
    smoothing = Smoothing.checked(mode, measurement, accel_psd, sigma_floor_mm, cov_scale, initial_speed_mm_s, gate)
    n_boxes, fi, ti = _box_frames(boxes, frame_index, track_index, 'track_index')
    times = _box_times(timestamps, fi, n_boxes)
    rows, starts = track_groups(ti, times)
    n_tracks = len(starts) - 1
    if state is not None:
        if (not isinstance(state, torch.Tensor) or state.dtype != torch.float64 or state.dim() != 3
                or state.shape[2] != TRACK_STATE_DOUBLES or state.shape[0] < n_tracks or not state.is_contiguous()):
            raise ValueError(f'state must be a contiguous float64 tensor [T, Jout, {TRACK_STATE_DOUBLES}] with T >= {n_tracks} '
                             '(new_track_state, or the state of a previous call)')
        starts = np.concatenate([starts, np.full(state.shape[0] - n_tracks, starts[-1], np.int32)])
    raw = locate_poses_in_frames(frames, boxes, model_path, cameras=cameras, frame_index=frame_index, return_uncertainty=True,
                                 **{k: kw[k] for k in _LOCATE_OPTIONS})
    device = raw.poses.device
    if state is None:
        state = new_track_state(n_tracks, raw.poses.shape[1], device)
    with torch.cuda.device(device):
        poses, velocity, covariance, used = _smooth_tracks(raw.poses, raw.covariance, times, rows, starts, smoothing, state)
    return TrackPoses(poses, velocity, covariance, used, raw, state, raw.joint_edges, raw.joint_names)


# ---- the same, with the tracks found on the device: frame-to-frame association (metro_associate_tracks) ----

class TrackTable(NamedTuple):
    """The tracks follow_poses_in_frames carries from call to call, on the device (new_track_table)."""
    state: torch.Tensor                  # float64 [T, Jout, 28]: the filter state per slot (track_poses_in_frames' `state`)
    ids: torch.Tensor                    # int32 [T]: the persistent id of the track in each slot, -1: the slot is free
    next_id: torch.Tensor                # int32 [1]: the next id to give


class FollowedPoses(NamedTuple):
    """What follow_poses_in_frames returns."""
    track_index: torch.Tensor            # int32 [n] on the device: the slot of every box, -1 untracked
    track_id: torch.Tensor               # int32 [n] on the device: the persistent id of its track, -1 untracked
    cost: torch.Tensor                   # float32 [n] mm: the cost at which a box continued its track (NaN: born here, or untracked)
    n_new: torch.Tensor                  # int32 [1] on the device: tracks born in this call
    n_dropped: torch.Tensor              # int32 [1] on the device: boxes left untracked (no free slot, or no finite joint)
    tracks: TrackTable                   # the table after this call (pass it to the next)
    smoothed: TrackPoses                 # track_poses_in_frames' result for that track_index; its state is tracks.state


def time_steps(timestamps) -> Tuple[np.ndarray, np.ndarray]:
    """The time-step CSR metro_associate_tracks reads, built on the host from one time per box: (step_rows int32 [n],
    step_starts int32 [S + 1]), step s owning the boxes step_rows[step_starts[s]:step_starts[s+1]] (in box order), the steps
    in ascending time, all boxes of one timestamp in one step.  ValueError for non-finite times and for more than 128 boxes
    on one timestamp."""
    from metro_pose3d_amd.heads import ASSOC_MAX
    ts = np.asarray(timestamps, np.float64).reshape(-1)
    if not np.isfinite(ts).all():
        raise ValueError('timestamps must be finite (seconds)')
    order = np.argsort(ts, kind='stable')
    new = np.concatenate([[True], ts[order][1:] != ts[order][:-1]]) if len(ts) else np.zeros(0, bool)
    starts = np.concatenate([np.flatnonzero(new), [len(ts)]]).astype(np.int32)
    sizes = np.diff(starts)
    if len(sizes) and sizes.max() > ASSOC_MAX:
        s = int(np.argmax(sizes))
        raise ValueError(f'{int(sizes[s])} boxes at time {ts[order][starts[s]]!r}: association takes at most {ASSOC_MAX} per '
                         'timestamp')
    return order.astype(np.int32), starts


def new_track_table(capacity: int, n_joints_out: int, device) -> TrackTable:
    """An empty table of `capacity` (1 to 128) track slots for follow_poses_in_frames / heads.associate_tracks: no state
    (new_track_state), every slot free (id -1), the first id to give 0."""
    from metro_pose3d_amd.heads import ASSOC_MAX
    if isinstance(capacity, (bool, np.bool_)) or not isinstance(capacity, (int, np.integer)) or not 1 <= capacity <= ASSOC_MAX:
        raise ValueError(f'capacity must be an integer from 1 to {ASSOC_MAX} (track slots), got {capacity!r}')
    return TrackTable(new_track_state(int(capacity), n_joints_out, device),
                      torch.full((int(capacity),), -1, dtype=torch.int32, device=device),
                      torch.zeros((1,), dtype=torch.int32, device=device))


def _check_track_table(tracks):
    from metro_pose3d_amd.heads import ASSOC_MAX, TRACK_STATE_DOUBLES
    ok =(isinstance(tracks, tuple) and len(tracks) == 3 and all(isinstance(t, torch.Tensor) for t in tracks)
          and tracks[0].dtype == torch.float64 and tracks[0].dim() == 3 and tracks[0].shape[2] == TRACK_STATE_DOUBLES
          and 1 <= tracks[0].shape[0] <= ASSOC_MAX and tracks[0].is_contiguous()
          and tracks[1].dtype == torch.int32 and tuple(tracks[1].shape) == (tracks[0].shape[0],) and tracks[1].is_contiguous()
          and tracks[2].dtype == torch.int32 and tracks[2].numel() == 1)
    if not ok:
        raise ValueError(f'tracks must be a TrackTable(state float64 [T, Jout, {TRACK_STATE_DOUBLES}], ids int32 [T], next_id int32 '
                         f'[1]) with 1 <= T <= {ASSOC_MAX} (new_track_table, or the table of a previous call)')


class BoneTable(NamedTuple):
    """The bone lengths a Follower(learn_bones=True) learns per track slot, on the device (new_bone_table)."""
    stats: torch.Tensor                  # float64 [T, E, 4]: per slot and skeleton edge S0 = sum 1/v, S1 = sum l/v, count, rejected
    ids: torch.Tensor                    # int32 [T]: the id of the track the slot's stats belong to (-1: nobody's)


def new_bone_table(capacity: int, n_edges: int, device) -> BoneTable:
    """An empty bone table for `capacity` (1 to 128) track slots and n_edges (1 to 64) skeleton edges: for
    heads.track_bone_lengths next to new_track_table's table of the same capacity."""
    from metro_pose3d_amd.heads import ASSOC_MAX, BONE_STAT_DOUBLES
    if isinstance(capacity, (bool, np.bool_)) or not isinstance(capacity, (int, np.integer)) or not 1 <= capacity <= ASSOC_MAX:
        raise ValueError(f'capacity must be an integer from 1 to {ASSOC_MAX} (track slots), got {capacity!r}')
    if isinstance(n_edges, (bool, np.bool_)) or not isinstance(n_edges, (int, np.integer)) or not 1 <= n_edges <= _lib.METRO_MAX_JOINTS:
        raise ValueError(f'n_edges must be an integer from 1 to {_lib.METRO_MAX_JOINTS} (skeleton edges), got {n_edges!r}')
    return BoneTable(torch.zeros((int(capacity), int(n_edges), BONE_STAT_DOUBLES), dtype=torch.float64, device=device),
                     torch.full((int(capacity),), -1, dtype=torch.int32, device=device))


def _checked_bone_table(bones, tracks: TrackTable, sk) -> BoneTable:
    from metro_pose3d_amd.heads import BONE_STAT_DOUBLES
    shape = (len(tracks.ids), len(sk.edges), BONE_STAT_DOUBLES)
    ok = (isinstance(bones, tuple) and len(bones) == 2 and all(isinstance(t, torch.Tensor) for t in bones)
          and bones[0].dtype == torch.float64 and tuple(bones[0].shape) == shape and bones[0].is_contiguous()
          and bones[1].dtype == torch.int32 and tuple(bones[1].shape) == shape[:1] and bones[1].is_contiguous()
          and bones[0].device == tracks.ids.device and bones[1].device == tracks.ids.device)
    if not ok:
        raise ValueError(f'bones must be a BoneTable(stats float64 {list(shape)}, ids int32 [{shape[0]}]) on the device of the track '
                         'table (new_bone_table, or the table of a previous call)')
    return BoneTable(*bones)


def follow_poses_in_frames(frames, boxes, model_path, cameras, frame_index, timestamps, tracks: Optional[TrackTable] = None,
                           capacity: int = 64, max_cost_mm: float = 300.0, clip_mm: float = 600.0,
                           min_joints: Optional[int] = None, max_age_s: float = 1.0, mode: str = 'smooth',
                           measurement: str = 'covariance', accel_psd: float = 4e6, sigma_floor_mm: float = 1.0,
                           cov_scale: float = 1.0, initial_speed_mm_s: float = 2000.0, gate=None,
                           scale_recovery: str = 'bone-lengths', bone_lengths=None, root_depth=None, coords: str = 'camera',
                           precision: Optional[str] = None, check_finite: Optional[bool] = None, views=None,
                           geometry: str = 'auto', pixel_format: str = 'rgb', color_matrix: str = 'bt601',
                           crop_dtype: str = 'float32') -> FollowedPoses:
    """track_poses_in_frames without a track_index: which box continues which track is decided on the device, from the
    forward's own outputs, between the forward and the smoothing launch -> FollowedPoses(track_index int32 [n], track_id
    int32 [n], cost [n], n_new [1], n_dropped [1], tracks: TrackTable, smoothed: TrackPoses).  Every other argument as there;
    a person detector's boxes per frame, in any order, are enough.  At most 128 boxes per timestamp and 128 track slots.

    The boxes are walked in time order over a table of track slots (heads.associate_tracks): at each timestamp the cost of a
    slot continuing in a box is the RMS distance in mm between the box's joints and the slot's constant-velocity prediction
    (the filter state advanced to the box's time), each joint capped at clip_mm, +inf from fewer than min_joints joints
    (None: half the output joints, rounded up) and for a slot last seen more than max_age_s before; slots and boxes are
    paired greedily, the smallest cost first, while it is below max_cost_mm (one box per slot, one slot per box); a box left
    over starts a new track in the lowest free slot, under the next id; with no slot free it stays untracked (-1, counted in
    n_dropped), as does a box with no finite joint.  The pairing is greedy, not an optimal assignment (Follower and
    follow_world_poses_in_frames take assignment='optimal'; heads.associate_tracks has both rules).  track_index is the
    slot (what track_poses_in_frames calls a track), track_id the identity that persists when slots are reused.
    max_cost_mm = 300, clip_mm = 600, max_age_s = 1 and the min_joints default are design choices, not measurements
    (heads.associate_tracks has the reasoning).
    tracks: None (a fresh table of `capacity` slots) or the table a previous call returned: tracks continue from it, a slot
    last seen more than max_age_s before this call's first box is retired first and free again, and the table is updated in
    place -- its ids, and its state with the FILTER state at each track's last box -- so a stream cut into calls gets the
    ids one long call gives.  `capacity` is read only when tracks is None.
    The poses must be absolute: scale_recovery 'metro' returns root-relative poses, in which all persons coincide, and is
    refused.
    One enqueue chain: track_poses_in_frames' own, with one metro_associate_tracks launch between the forward and
    metro_smooth_tracks, which reads the device CSR that launch wrote and tracks.state; track_index is never read on the
    host, and the call's one synchronisation stays the finite screen.
    ValueError before any launch for more than 128 boxes on one timestamp, capacity outside [1, 128], a tracks that is no
    table, scale_recovery 'metro', max_cost_mm, clip_mm, min_joints or max_age_s out of range, and whatever
    track_poses_in_frames refuses."""
    return _follow_poses(frames, boxes, model_path, cameras, frame_index, timestamps, tracks, capacity,
                         *_camera_groups(locals(), 'greedy'))


_CALL_OPTIONS = ('views', 'geometry', 'precision', 'check_finite', 'pixel_format', 'color_matrix', 'crop_dtype')    # _checked_call's
_LOCATE_OPTIONS = ('scale_recovery', 'bone_lengths', 'root_depth', 'coords') + _CALL_OPTIONS


def _camera_groups(kw: dict, assignment):
    """The keywords of follow_poses_in_frames (`kw` holds them by name: the call's locals(), or Follower's) checked once, here ->
    (heads.Association, heads.Smoothing, the keywords handed on to locate_poses_in_frames)."""
    from metro_pose3d_amd.heads import Association, Smoothing
    association = Association.checked(kw['max_cost_mm'], kw['clip_mm'], kw['min_joints'], kw['max_age_s'], assignment)
    smoothing = Smoothing.checked(*(kw[k] for k in Smoothing._fields))
    if kw['scale_recovery'] == 'metro':
        raise ValueError("scale_recovery='metro' returns root-relative poses, in which all persons coincide: following needs "
                         "absolute poses ('bone-lengths' or 'true-root-depth')")
    return association, smoothing, {k: kw[k] for k in _LOCATE_OPTIONS}


def _check_tracks_or_capacity(tracks, capacity) -> None:
    """A table to continue, or the capacity of a fresh one: checked before any launch."""
    if tracks is None:
        new_track_table(capacity, 1, 'cpu')
    else:
        _check_track_table(tracks)


def _follow_poses(frames, boxes, model_path, cameras, frame_index, timestamps, tracks, capacity, association, smoothing, locate):
    """follow_poses_in_frames on checked groups (heads.Association with its assignment rule -- 'greedy' there, Follower passes its
    own -- and heads.Smoothing); locate: the keywords handed on to locate_poses_in_frames, none of them scale_recovery 'metro'."""
    from metro_pose3d_amd.heads import _associate_tracks, _smooth_tracks
    n_boxes, fi = _box_frames(boxes, frame_index)
    times = _box_times(timestamps, fi, n_boxes)
    step_rows, step_starts = time_steps(times)
    _check_tracks_or_capacity(tracks, capacity)
    raw = locate_poses_in_frames(frames, boxes, model_path, cameras=cameras, frame_index=frame_index, return_uncertainty=True, **locate)
    device = raw.poses.device
    tracks = new_track_table(capacity, raw.poses.shape[1], device) if tracks is None else TrackTable(*tracks)
    with torch.cuda.device(device):
        found = _associate_tracks(raw.poses, raw.covariance, times, step_rows, step_starts, *tracks, association, smoothing)
        poses, velocity, covariance, used = _smooth_tracks(raw.poses, raw.covariance, times, found.rows, found.starts, smoothing,
                                                           tracks.state)
    smoothed = TrackPoses(poses, velocity, covariance, used, raw, tracks.state, raw.joint_edges, raw.joint_names)
    return FollowedPoses(found.track_index, found.track_id, found.cost, found.n_new, found.n_dropped, tracks, smoothed)


# ---- several calibrated cameras over time: persons matched across cameras, triangulated, followed and smoothed in the world ----

MAX_WORLD_FRAMES = 64                # frames (camera exposures) of one follow_world_poses_in_frames call


class SmoothedWorldPoses(NamedTuple):
    """The smoothing launch's outputs in FollowedWorldPoses, one row per person found."""
    poses: torch.Tensor                  # float32 [P, Jout, 3] world mm: filtered / smoothed (untracked persons: world.poses)
    velocity: torch.Tensor               # float32 [P, Jout, 3] mm/s (NaN for untracked persons)
    covariance: torch.Tensor             # float32 [P, Jout, 3, 3] mm^2 of the position estimate (untracked persons: their R)
    used: torch.Tensor                   # uint8 [P, Jout]: 1 where the person's joint entered the update
    state: torch.Tensor                  # float64 [T, Jout, 28]: tracks.state


class FollowedWorldPoses(NamedTuple):
    """What follow_world_poses_in_frames returns; P = the persons found (one per person and time step)."""
    person_index: torch.Tensor           # int32 [n] on the device: the person of every box, numbered by their lowest box
    cost: torch.Tensor                   # float32 [n, n] mm: match_poses_in_frames' cost, +inf also across time steps
    n_pairs: torch.Tensor                # int32 [n, n]
    world: WorldPoses                    # the triangulated poses, one row per person found
    world_covariance: torch.Tensor       # float32 [P, Jout, 9] mm^2: covariance of every triangulated joint, NaN where the joint is
    person_step: torch.Tensor            # int32 [P]: the time step of the person (index into the sorted distinct timestamps), -1: none
    track_index: torch.Tensor            # int32 [P]: the slot of every person, -1 untracked
    track_id: torch.Tensor               # int32 [P]: the persistent id of its track, -1 untracked
    track_cost: torch.Tensor             # float32 [P] mm: the cost at which a person continued its track (NaN: born here, or untracked)
    n_new: torch.Tensor                  # int32 [1]: tracks born in this call
    n_dropped: torch.Tensor              # int32 [1]: persons of the steps left untracked (no free slot, or no finite joint)
    tracks: TrackTable                   # the table after this call (pass it to the next)
    smoothed: SmoothedWorldPoses


def follow_world_poses_in_frames(frames, boxes, model_path, cameras, frame_index, timestamps, tracks: Optional[TrackTable] = None,
                                 capacity: int = 64, match_max_cost_mm: float = 200.0, match_clip_mm: float = 500.0,
                                 match_min_joints: Optional[int] = None, weights: str = 'covariance', min_angle_deg: float = 2.0,
                                 max_cost_mm: float = 300.0, clip_mm: float = 600.0, min_joints: Optional[int] = None,
                                 max_age_s: float = 1.0, mode: str = 'smooth', measurement: str = 'covariance',
                                 accel_psd: float = 4e6, sigma_floor_mm: float = 1.0, cov_scale: float = 1.0,
                                 initial_speed_mm_s: float = 2000.0, gate=None, views=None, precision: Optional[str] = None,
                                 check_finite: Optional[bool] = None, geometry: str = 'auto', pixel_format: str = 'rgb',
                                 color_matrix: str = 'bt601', crop_dtype: str = 'float32',
                                 assignment: str = 'greedy') -> FollowedWorldPoses:
    """A calibrated rig's video: a person detector's boxes per camera and per exposure, unordered and without identity ->
    FollowedWorldPoses: the boxes matched across the cameras of each exposure (match_poses_in_frames), every person found
    triangulated in the world with the covariance of each joint, the persons followed from exposure to exposure under ids that
    persist (follow_poses_in_frames' association, here on world poses: neither bone lengths nor a root depth are needed) and
    smoothed by the Kalman / RTS launch with the triangulation's covariance as measurement noise.

    frames: the exposures of all cameras, one frame each; cameras: a list with one Camera per frame (a camera's Camera repeats
    for each of its exposures); frame_index [n]: the frame of each box, host integers.  timestamps: seconds, one per frame or
    one per box (follow_poses_in_frames' rule); the frames that share a timestamp form one time step, one exposure of the rig.
    At most 128 boxes and 64 frames per call.
    match_max_cost_mm, match_clip_mm, match_min_joints, weights and min_angle_deg are match_poses_in_frames' max_cost_mm,
    clip_mm, min_joints, weights and min_angle_deg; max_cost_mm, clip_mm, min_joints, max_age_s, mode, measurement, accel_psd,
    sigma_floor_mm, cov_scale, initial_speed_mm_s and gate are follow_poses_in_frames'; all keep their defaults there, which
    are design choices, not measurements (heads.view_affinity, heads.associate_tracks and heads.smooth_tracks have the
    reasoning).  tracks and capacity as in follow_poses_in_frames: the table carries over between calls, so a stream cut into
    calls at step boundaries gets the ids and filter states one long call gives.
    assignment: 'greedy' (the default: the smallest cost first) or 'optimal' (the admissible pairs of the largest total gain
    max_cost_mm - cost, which keeps the ids of persons close together where greedy swaps them), heads.associate_tracks' rule.
    Two boxes of different time steps are never matched (their cost is +inf, as for two boxes of one frame), so a person found
    lives in one step: P counts persons per step.  With weights 'uniform' exactly meeting rays give a zero covariance;
    sigma_floor_mm keeps the measurement noise positive definite.
    A person seen by one camera only has NaN world joints and no step (person_step -1): it is in no step of the association,
    stays untracked (track_index -1) and its track is bridged by the motion model until max_age_s
    (follow_rig_poses_in_frames is this call with such a person's rays fed to its track instead).  A person seen by several
    cameras none of whose joints could be triangulated is in its step, untracked and counted in n_dropped.
    One enqueue chain: match_poses_in_frames' own up to the forward, then, with no host work in between and all over the upper
    bound of n persons, metro_view_affinity_steps, metro_cluster_views, metro_triangulate_joints_cov, metro_person_steps,
    metro_associate_tracks and metro_smooth_tracks; the call's one synchronisation stays the finite screen, which also brings
    the number of persons, to which the per-person outputs are sliced.
    ValueError before any launch for more than 128 boxes or 64 frames, cameras=None, timestamps that are not finite or match
    neither frames nor boxes, capacity outside [1, 128], a tracks that is no table or has another joint count than the model,
    and whatever match_poses_in_frames and follow_poses_in_frames refuse of their keywords."""
    return _follow_world(frames, boxes, model_path, cameras, frame_index, timestamps, tracks, capacity,
                         *_world_groups(locals(), assignment, 'skip'))[0]


SINGLE_VIEWS = ('rays', 'skip')


def _world_groups(kw: dict, assignment, single_view):
    """The keywords of follow_world_poses_in_frames / follow_rig_poses_in_frames (`kw` holds them by name: the call's locals(), or
    Follower's) checked once, here -> (heads.Matching, heads.Triangulation, heads.Association -- with the ray depth sigma for
    single_view 'rays' only --, heads.Smoothing, the keywords handed on to _checked_call)."""
    from metro_pose3d_amd.heads import Association, Matching, Smoothing, Triangulation
    if not isinstance(single_view, str) or single_view not in SINGLE_VIEWS:
        raise ValueError(f"single_view must be 'rays' or 'skip', got {single_view!r}")
    rays = single_view == 'rays'
    association = Association.checked(kw['max_cost_mm'], kw['clip_mm'], kw['min_joints'], kw['max_age_s'], assignment,
                                      kw.get('ray_depth_sigma_mm'), rays)
    if rays and kw['measurement'] == 'isotropic':
        raise ValueError("single_view='rays' needs measurement='covariance': an isotropic R would ignore the ray's shape and "
                         'pin the depth along it')
    triangulation = Triangulation.checked(kw['weights'], kw['min_angle_deg'])
    matching = Matching.checked(kw['match_max_cost_mm'], kw['match_clip_mm'], kw['match_min_joints'])
    smoothing = Smoothing.checked(*(kw[k] for k in Smoothing._fields))
    return matching, triangulation, association, smoothing, {k: kw[k] for k in _CALL_OPTIONS}


def _follow_world(frames, boxes, model_path, cameras, frame_index, timestamps, tracks, capacity, matching, triangulation, association,
                  smoothing, call_options, bones=None):
    """follow_world_poses_in_frames and follow_rig_poses_in_frames on checked groups (_world_groups) -> (FollowedWorldPoses, None
    or (single_view uint8 [P], ray_depth float32 [P, Jout], n_unplaced int32 [1]) of the 'rays' chain -- the one whose association
    holds a ray depth sigma --, the bone table).
    bones: None (nothing is learned: the chain is what it was), True (a fresh table) or the BoneTable of the previous call:
    one metro_track_bone_lengths launch after the smoothing launch accumulates every followed person's bone lengths from the
    triangulation's own poses and covariance."""
    from metro_pose3d_amd.heads import (MATCH_MAX_BOXES, _associate_tracks, _smooth_tracks, person_rays, person_steps, person_steps_labels,
                                        track_bone_lengths)
    n_boxes, fi = _box_frames(boxes, frame_index)
    if n_boxes > MATCH_MAX_BOXES:
        raise ValueError(f'{n_boxes} boxes: matching takes at most {MATCH_MAX_BOXES} per call')
    if len(np.unique(fi)) > MAX_WORLD_FRAMES:
        raise ValueError(f'{len(np.unique(fi))} frames: at most {MAX_WORLD_FRAMES} per call')
    _check_rig(cameras, fi, n_boxes)
    times = _box_times(timestamps, fi, n_boxes)
    step_times, box_step = np.unique(times, return_inverse=True)
    _check_tracks_or_capacity(tracks, capacity)
    call = _checked_call(frames, boxes, fi, 'world', **call_options)
    sk = _model_skeleton(model_path)
    _check_min_joints(association.min_joints, sk)
    if tracks is not None and tracks[0].shape[1] != sk.n_out:
        raise ValueError(f'tracks.state holds {tracks[0].shape[1]} joints, the model has {sk.n_out}')
    device = _call_device(call.boxes, call.frames)
    tracks = new_track_table(capacity, sk.n_out, device) if tracks is None else TrackTable(*tracks)
    if bones is not None:
        bones = new_bone_table(len(tracks.ids), len(sk.edges), device) if bones is True else _checked_bone_table(bones, tracks, sk)
    _check_min_joints(matching.min_joints, sk)
    if len(call.boxes) == 0:                                # no boxes: no launch
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=device)
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=device)
        smoothed = SmoothedWorldPoses(f32(0, sk.n_out, 3), f32(0, sk.n_out, 3), f32(0, sk.n_out, 3, 3),
                                      torch.zeros((0, sk.n_out), dtype=torch.uint8, device=device), tracks.state)
        return (FollowedWorldPoses(*_no_persons(sk, device), f32(0, sk.n_out, 9), i32(0), i32(0), i32(0), f32(0), i32(1), i32(1),
                                   tracks, smoothed), None, bones)
    chain = _enqueue_world(call, model_path, cameras, fi, triangulation, matching=matching, step_index=box_step, covariance=True)
    places, extra = chain.places.reshape(-1), None
    with torch.cuda.device(device):                         # between the triangulation and metro_place_poses, nothing read back
        poses, cov = chain.poses, chain.covariance          # the triangulation's own: NaN for a person one camera sees
        if association.ray_depth_sigma_mm is not None:
            person_step, person_times, step_rows, step_starts, single_box = person_steps_labels(chain.labels, chain.n_persons, box_step,
                                                                                                step_times)
            rays = person_rays(chain.coords01, chain.cov01, places, single_box, chain.eng.spec, chain.nv, triangulation.weights)
            found = _associate_tracks(poses, cov, person_times, step_rows, step_starts, *tracks, association, smoothing, (single_box, rays))
            poses, cov = found.poses, found.covariance      # copies with the placed joints: the triangulation's own stay as they are
            extra = ((single_box >= 0).to(torch.uint8), found.ray_depth, found.n_unplaced)
        else:
            person_step, person_times, step_rows, step_starts = person_steps(chain.rows, chain.starts, chain.n_persons, box_step,
                                                                             step_times, chain.nv)
            found = _associate_tracks(poses, cov, person_times, step_rows, step_starts, *tracks, association, smoothing)
        smooth = _smooth_tracks(poses, cov, person_times, found.rows, found.starts, smoothing, tracks.state)
        if bones is not None:                               # the raw measurements, not the smoothed rows: those are correlated in time
            track_bone_lengths(chain.poses, chain.covariance if smoothing.measurement == 'covariance' else None, found.rows, found.starts,
                               tracks.ids, bones.stats, bones.ids, sk.edges, sk.edge_mirror(), sigma_floor_mm=smoothing.sigma_floor_mm,
                               cov_scale=smoothing.cov_scale)
    world, p = _finish_world(call, chain)
    if extra is not None:
        extra = (extra[0][:p], extra[1][:p], extra[2])
    return (FollowedWorldPoses(chain.labels, chain.cost, chain.n_pairs, world, chain.covariance[:p], person_step[:p], found.track_index[:p],
                               found.track_id[:p], found.cost[:p], found.n_new, found.n_dropped, tracks,
                               SmoothedWorldPoses(*(t[:p] for t in smooth), tracks.state)), extra, bones)


class FollowedRigPoses(NamedTuple):
    """What follow_rig_poses_in_frames returns: FollowedWorldPoses' fields in their order, then the single-view ones."""
    person_index: torch.Tensor
    cost: torch.Tensor
    n_pairs: torch.Tensor
    world: WorldPoses                    # the triangulated poses; NaN for a person one camera sees, placed or not
    world_covariance: torch.Tensor
    person_step: torch.Tensor            # int32 [P]: with single_view='rays' a person one camera sees has its step too
    track_index: torch.Tensor
    track_id: torch.Tensor
    track_cost: torch.Tensor             # float32 [P] mm: for a person one camera sees, the RMS distance of the track's joints from its rays
    n_new: torch.Tensor
    n_dropped: torch.Tensor              # int32 [1]: persons SEVERAL cameras see left untracked
    tracks: TrackTable
    smoothed: SmoothedWorldPoses         # of a person one camera sees: the track's joints updated across the rays, bridged along them
    single_view: torch.Tensor            # uint8 [P]: 1 where the person is seen by one camera and went into the association as rays
    ray_depth: torch.Tensor              # float32 [P, Jout] mm: the depth along its ray at which a joint was placed, NaN elsewhere
    n_unplaced: torch.Tensor             # int32 [1]: persons one camera sees that no track continued in (never born: no depth)


def follow_rig_poses_in_frames(frames, boxes, model_path, cameras, frame_index, timestamps, tracks: Optional[TrackTable] = None,
                               capacity: int = 64, match_max_cost_mm: float = 200.0, match_clip_mm: float = 500.0,
                               match_min_joints: Optional[int] = None, weights: str = 'covariance', min_angle_deg: float = 2.0,
                               max_cost_mm: float = 300.0, clip_mm: float = 600.0, min_joints: Optional[int] = None,
                               max_age_s: float = 1.0, mode: str = 'smooth', measurement: str = 'covariance',
                               accel_psd: float = 4e6, sigma_floor_mm: float = 1.0, cov_scale: float = 1.0,
                               initial_speed_mm_s: float = 2000.0, gate=None, views=None, precision: Optional[str] = None,
                               check_finite: Optional[bool] = None, geometry: str = 'auto', pixel_format: str = 'rgb',
                               color_matrix: str = 'bt601', crop_dtype: str = 'float32', assignment: str = 'greedy',
                               single_view: str = 'rays', ray_depth_sigma_mm: float = 1000.0) -> FollowedRigPoses:
    """follow_world_poses_in_frames in which a person that only ONE camera sees keeps feeding its track -> FollowedRigPoses.
    Every parameter up to `assignment` is follow_world_poses_in_frames', with its default.

    There, such a person has NaN world joints and no step: its track coasts on the motion model while a camera looks straight at
    the person, and after max_age_s it is retired and the person returns under a new id.  But one camera gives a ray per joint
    and a lateral variance per ray, which pins the joint in two of three directions; the track's own prediction supplies the
    third.  single_view='rays' (the default): the person gets its step (metro_person_steps_labels in place of
    metro_person_steps) and its rays (metro_person_rays), and metro_associate_tracks_rays in place of the association entry
    costs it against the tracks by the distance of their predicted joints from the rays, assigns it among the triangulated
    persons under either rule, and places every joint at the foot of the perpendicular from the predicted joint onto its ray
    with R = sigma2 tau^2 (I - d d^T) + ray_depth_sigma_mm^2 d d^T (heads.associate_tracks_rays has the model), which
    metro_smooth_tracks, unchanged, then reads.  The association runs on copies of the triangulation's poses and covariance:
    world.poses and world_covariance stay the triangulation's own, NaN for such a person; smoothed holds its updated joints.
    The cost is blind along the ray, and such a person never STARTS a track (no depth): unassigned it is untracked and counted
    in n_unplaced.  Still one synchronisation, and no host work after the forward.
    single_view='skip': exactly the chain follow_world_poses_in_frames enqueues and its tensors; single_view all 0, ray_depth
    NaN, n_unplaced 0.
    ray_depth_sigma_mm = 1000 is a design choice, not a measurement (heads.associate_tracks_rays has the reasoning): large
    against the predicted position variance along the ray, so the depth stays the motion model's; small enough that the fp32
    rounding of R stays far below sigma_floor_mm^2.
    ValueError before any launch for whatever follow_world_poses_in_frames refuses, an unknown single_view, ray_depth_sigma_mm
    not finite and > 0, and measurement='isotropic' together with 'rays'."""
    return _rig_poses(*_follow_world(frames, boxes, model_path, cameras, frame_index, timestamps, tracks, capacity,
                                     *_world_groups(locals(), assignment, single_view))[:2])


def _rig_poses(out: FollowedWorldPoses, extra) -> FollowedRigPoses:
    """_follow_world's pair as FollowedRigPoses; extra None (the 'skip' chain): single_view all 0, ray_depth NaN, n_unplaced 0."""
    if extra is None:
        p, device = len(out.person_step), out.person_step.device
        extra = (torch.zeros((p,), dtype=torch.uint8, device=device),
                 torch.full((p, out.smoothed.poses.shape[1]), float('nan'), dtype=torch.float32, device=device),
                 torch.zeros((1,), dtype=torch.int32, device=device))
    return FollowedRigPoses(*out, *extra)


# ---- the boxes of the next frames from the track table: crops between the key frames of a detector (metro_predict_boxes) ----

class PredictedBoxes(NamedTuple):
    """What predict_boxes_in_frames returns; every tensor on the table's device, n rows: the predicted boxes frame-major, then by
    slot, then the detections that were kept, in their given order."""
    boxes: torch.Tensor                  # float64 [n, 4] (x, y, w, h): `boxes` of the next call
    frame_index: torch.Tensor            # int32 [n]: its `frame_index`
    track_index: torch.Tensor            # int32 [n]: the slot of a predicted box, -1 for a detection
    track_id: torch.Tensor               # int32 [n]: its persistent id, -1 for a detection
    detection: torch.Tensor              # int32 [n]: the index of a detection in `detections`, -1 for a predicted box
    n_joints: torch.Tensor               # int32 [n]: the joints the predicted box was built from, -1 for a detection
    n_predicted: int                     # the first n_predicted rows are predicted boxes
    n_suppressed: int                    # detections left out because a predicted box of their frame covers them
    n_bad_detections: int                # detections left out because they are no boxes (non-finite, w or h <= 0)
    dense_boxes: torch.Tensor            # float64 [F, T, 4]: the box of every (frame, slot), NaN where there is none
    dense_joints: torch.Tensor           # int32 [F, T]: its visible joints; -1: the slot is free or older than max_age_s


def frame_sizes(frames, pixel_format: str = 'rgb') -> np.ndarray:
    """int32 [F, 2], the (W, H) in pixels of every frame as the calls above take them: [H, W, 3] for 'rgb' and 'bgr', the
    [H*3/2, W] layouts of 'nv12' and 'i420' or their plane tuples (Y [H, W] first).  Metadata only: host or device frames,
    nothing is copied.  ValueError for a layout the format does not take."""
    if pixel_format not in PIXEL_FORMATS:
        raise ValueError(f"pixel_format must be 'rgb', 'bgr', 'nv12' or 'i420', got {pixel_format!r}")
    from metro_pose3d_amd.frame_formats import _checked_frames
    items = frames.items if isinstance(frames, _FrameSet) else _checked_frames(frames, pixel_format, 'bt601').items
    planar = [_planar(k, f, pixel_format, 'bt601') for k, f in enumerate(items)]
    return np.asarray([[p.w, p.h] for p in planar], np.int32).reshape(-1, 2)


def predict_boxes_in_frames(tracks: TrackTable, cameras, frame_sizes, timestamps, coords: str = 'camera', detections=None,
                            detection_frame_index=None, expand: float = 1.25, n_sigma: float = 2.0, max_sigma_mm: float = 300.0,
                            min_joints: Optional[int] = None, max_age_s: float = 1.0, near_mm: float = 100.0,
                            min_side_px: float = 8.0, iou_max: float = 0.3, accel_psd: float = 4e6,
                            clip: bool = True) -> PredictedBoxes:
    """Where the tracked persons are about to be, as person boxes: the table a follow_poses_in_frames /
    follow_world_poses_in_frames call returned + the calibrated cameras, sizes (frame_sizes) and times of the NEXT frames ->
    PredictedBoxes(boxes float64 [n, 4], frame_index, track_index, track_id, detection, n_joints int32 [n], n_predicted,
    n_suppressed, n_bad_detections, dense_boxes, dense_joints), every tensor on the table's device.  Between the key frames of
    a person detector the follow_* calls run on these boxes alone; on a key frame the detector's boxes come along as
    `detections` and a person the detector missed on some camera still gets a crop.

    cameras: one Camera for every frame or a list with one per frame, as the follow_* call had them; timestamps: one time
    per frame, seconds on the clock of the table; coords: 'camera' for a table of follow_poses_in_frames(coords='camera'),
    whose state is in the camera's frame (one camera: every frame sees the same table), 'world' for
    follow_world_poses_in_frames' or coords='world' tables.  'crop' is refused: a crop's own camera differs from box to box.
    heads.predict_boxes has the rule (one box per frame and live track around the filter's predicted joints, the margin from
    their predicted covariance) and the reasoning behind expand, n_sigma, max_sigma_mm, near_mm, min_side_px and iou_max,
    which are design choices, not measurements; max_age_s and accel_psd are the follow_* calls' own and should be theirs;
    min_joints None: half the output joints, rounded up.
    detections float [m, 4] with detection_frame_index [m] (host data or CUDA tensors; None: frame 0), at most 4096: kept,
    after the predicted rows and in their order, unless a predicted box of their frame overlaps them with an intersection
    over union of iou_max or more.  Suppression among the detections themselves is the detector's.
    The table is read, never written.  Two launches and ONE synchronisation: the call reads the five counts to slice the
    rows; a detection frame index outside [0, F) raises ValueError there.
    The rows go unchanged into follow_poses_in_frames, follow_world_poses_in_frames and locate_poses_in_frames as boxes and
    frame_index (CUDA tensors: geometry='device') and, with person_index=track_index, into triangulate_poses_in_frames.
    ValueError before any launch for a tracks that is no table, cameras=None, coords 'crop', frame sizes below 1, times that
    are not one finite value per frame, more than 64 frames or 4096 detections, and any keyword out of range."""
    from metro_pose3d_amd.heads import predict_boxes, prediction_params
    if coords not in ('camera', 'world'):
        raise ValueError(f"coords must be 'camera' or 'world' (a crop has no calibrated camera of its own frame), got {coords!r}")
    prediction_params(expand, n_sigma, max_sigma_mm, min_joints, max_age_s, near_mm, min_side_px, iou_max, accel_psd)
    _check_track_table(tracks)
    tracks = TrackTable(*tracks)
    if cameras is None:
        raise ValueError('cameras: predicting boxes needs calibrated cameras (one Camera, or one per frame)')
    sizes = np.asarray(_host_array(frame_sizes))
    if sizes.ndim != 2 or sizes.shape[1] != 2 or not 1 <= len(sizes) <= _lib.METRO_MAX_FRAMES:
        raise ValueError(f'frame_sizes must be [F, 2] (W, H) with 1 <= F <= {_lib.METRO_MAX_FRAMES} (frames.frame_sizes), got '
                         f'{sizes.shape}')
    rec = pack_frame_cameras(cameras, len(sizes))
    rows = predict_boxes(tracks.state, tracks.ids, rec, sizes, _host_array(timestamps), coords, detections, detection_frame_index,
                         expand, n_sigma, max_sigma_mm, min_joints, max_age_s, near_mm, min_side_px, iou_max, accel_psd, clip)
    n, n_predicted, n_suppressed, n_bad, n_bad_frames = rows.counts.tolist()         # the call's one synchronisation
    _raise_on_bad_frames(n_bad_frames, 0 if detections is None else len(detections), len(sizes))
    return PredictedBoxes(rows.boxes[:n], rows.frame_index[:n], rows.track_index[:n], rows.track_id[:n], rows.detection[:n],
                          rows.n_joints[:n], n_predicted, n_suppressed, n_bad, rows.dense_boxes, rows.dense_joints)


# ---- the tracks as the prior of the crops' heat-map posterior: predict -> locate between key frames (metro_plan_bind_track_prior) ----

class TrackedFramePoses(NamedTuple):
    """What locate_tracked_poses_in_frames returns; every tensor on the call's device."""
    plain: FramePoses                    # locate_poses_in_frames' result for these boxes, bit for bit
    posterior: FramePoses                # the same placement and merge on the posterior means (covariance and peak None)
    posterior_covariance: torch.Tensor   # float32 [n, Jout, 3, 3] mm^2 in the requested coords, views averaged
    log_evidence: torch.Tensor           # float32 [n, V, Jout]: per view row, unmerged; exactly 0 where reason != 0
    peak: torch.Tensor                   # float32 [n, V, Jout]: the largest posterior probability of a voxel
    reason: torch.Tensor                 # int32 [n, V, Jout]: 0 prior given, else why not (heads.REASONS)


def _device_slots(track_index, n: int, device: torch.device) -> torch.Tensor:
    """track_index (host integers or a CUDA integer tensor, one per box) -> int32 [n] on the device, without a synchronisation."""
    if isinstance(track_index, torch.Tensor) and track_index.is_cuda:
        if track_index.device != device:
            raise ValueError(f'track_index is on {track_index.device}, the call runs on {device}')
        if track_index.is_floating_point() or track_index.is_complex() or track_index.dtype == torch.bool:
            raise ValueError(f'track_index must hold integers, got {track_index.dtype}')
        if track_index.numel() != n:
            raise ValueError(f'track_index must hold {n} values (one per box), got {track_index.numel()}')
        ti = track_index.reshape(n)
        if ti.dtype != torch.int32:             # out-of-range values stay out of range through the cast
            ti = ti.to(torch.int64).clamp(-1, _lib.METRO_ASSOC_MAX).to(torch.int32)
        return ti.contiguous()
    ti = np.asarray(_host_array(track_index)).reshape(-1)
    if ti.dtype.kind not in 'iu' or len(ti) != n:
        raise ValueError(f'track_index must hold {n} integers (one per box; -1: no track), got {ti.dtype} [{len(ti)}]')
    return _upload(np.clip(ti.astype(np.int64), -1, _lib.METRO_ASSOC_MAX).astype(np.int32), device)


def _device_times(timestamps, frame_index, n: int, device: torch.device) -> torch.Tensor:
    """timestamps (host data: one per box, or one per frame looked up through frame_index) -> float64 [n] on the device.  A
    host frame index is looked up on the host (_box_times, with its checks); a CUDA one on the device, clamped to the table
    (the call's frame check reports an index outside it)."""
    if isinstance(frame_index, torch.Tensor) and frame_index.is_cuda:
        ts = np.asarray(_host_array(timestamps), np.float64).reshape(-1)
        if not np.isfinite(ts).all() or len(ts) == 0:
            raise ValueError('timestamps must be finite (seconds), one per box or one per frame')
        d_ts = _upload(ts, device)
        if len(ts) == n:
            return d_ts
        return d_ts.index_select(0, frame_index.reshape(-1).to(torch.int64).clamp(0, len(ts) - 1)).contiguous()
    fi = np.zeros(n, np.int64) if frame_index is None else np.asarray(_host_array(frame_index), np.int64).reshape(-1)
    if len(fi) != n:
        raise ValueError(f'frame_index must hold one value per box ({n}), got {len(fi)}')
    return _upload(np.ascontiguousarray(_box_times(timestamps, fi, n)), device)


def locate_tracked_poses_in_frames(frames, boxes, model_path, cameras, tracks: TrackTable, track_index, frame_index, timestamps,
                                   table_coords: str = 'camera', depth: str = 'none', accel_psd: float = 4e6,
                                   max_age_s: float = 1.0, near_mm: float = 100.0, sigma_floor_mm: float = 30.0,
                                   cov_scale: float = 1.0, scale_recovery: str = 'bone-lengths', bone_lengths=None,
                                   root_depth=None, coords: str = 'camera', precision: Optional[str] = None,
                                   check_finite: Optional[bool] = None, views=None, geometry: str = 'auto',
                                   pixel_format: str = 'rgb', color_matrix: str = 'bt601',
                                   crop_dtype: str = 'float32') -> TrackedFramePoses:
    """locate_poses_in_frames with each person's own track as the prior of each crop's heat-maps -> TrackedFramePoses(plain,
    posterior, posterior_covariance, log_evidence, peak, reason).  Between the key frames of a detector, predict_boxes_in_frames
    says where to cut the crops; this call also tells the network's read-out where the track expects every joint: a two-peaked
    joint (a left/right swap, a second person in the crop) resolves to the peak the track agrees with, and exp(log_evidence)
    is the probability the heat-map gives to the track's region -- the value a tracker gates a measurement with.

    frames, boxes, cameras, frame_index and every keyword from scale_recovery on are locate_poses_in_frames'; cameras must be
    calibrated (a prior is projected through the crop's virtual camera).  tracks: the TrackTable a follow_* call returned,
    read, never written.  track_index [n]: the table slot of each box, host integers or a CUDA integer tensor (-1, or a slot
    outside the table: no prior for that box); timestamps: seconds on the clock of the table, host data, one per box or one
    per frame looked up through frame_index.  boxes, frame_index and track_index may be the CUDA tensors of PredictedBoxes
    as they are.  table_coords: 'camera' or 'world', the frame the table lives in (follow_poses_in_frames' coords;
    'world' for follow_world_poses_in_frames); it need not be `coords`, the frame of the poses returned.
    depth, accel_psd, max_age_s, near_mm, sigma_floor_mm, cov_scale: heads.track_prior_params.  The defaults sigma_floor_mm =
    30, cov_scale = 1, near_mm = 100 and depth = 'none' are design choices, not measurements (the reasoning is there);
    max_age_s and accel_psd are the follow_* calls' own and should be theirs.
    One enqueue chain and ONE synchronisation, locate_poses_in_frames' own with the track prior bound to the forward
    (Engine.forward_track_posterior: one more small launch, which writes the prior rows of every crop row from the table --
    track_index and the times repeated per view on the device, a flipped view reading the mirror joints -- and the posterior
    launch).  `plain` is locate_poses_in_frames' result, bit for bit.  `posterior` is placed by the same metro_place_poses and
    metro_merge_views launches on a head-order copy of coords01 whose output joints are replaced by the posterior means (head
    joints the output order does not carry keep their plain mean; scale_recovery 'metro' roots the posterior means as
    inference.posterior_to_metric does).  posterior_covariance is the posterior's covariance in `coords`, by
    metro_place_covariances as FramePoses.covariance.  log_evidence, peak and reason stay per view row.
    Limits: the prior is only as good as the track -- a track that follows the wrong person pulls the posterior to that
    person, and log_evidence is the figure to gate on; xy rests on the heatmap_to_image convention every keypoint here rests
    on; z (depth='root') is anchored at the plain root mean of the same forward; sharded calls are not served.
    ValueError before any launch for cameras=None, a tracks that is no table or whose joints are not the model's, table_coords
    other than 'camera' / 'world', any keyword out of range, and whatever locate_poses_in_frames refuses."""
    from metro_pose3d_amd.heads import track_prior_params
    call = _checked_call(frames, boxes, frame_index, coords, views, geometry, precision, check_finite, pixel_format,
                         color_matrix, crop_dtype)
    if table_coords not in ('camera', 'world'):
        raise ValueError(f"table_coords must be 'camera' or 'world' (the frame the track table lives in), got {table_coords!r}")
    prior = dict(coords=table_coords, depth=depth, accel_psd=accel_psd, max_age_s=max_age_s, near_mm=near_mm,
                 sigma_floor_mm=sigma_floor_mm, cov_scale=cov_scale)
    track_prior_params(**prior)
    if cameras is None:
        raise ValueError('cameras: a track prior is projected through the crop\'s virtual camera and needs calibrated cameras')
    _check_track_table(tracks)
    tracks = TrackTable(*tracks)
    sk = _model_skeleton(model_path)
    if tracks.state.shape[1] != sk.n_out:
        raise ValueError(f'the track table holds {tracks.state.shape[1]} joints, the model returns {sk.n_out}')
    on_device = isinstance(bone_lengths, torch.Tensor) and bone_lengths.is_cuda
    n = len(call.boxes)
    targets, per_pose, root_z = _placement_targets(scale_recovery, cameras, n, len(sk.head_edges), bone_lengths, root_depth,
                                                   _call_device(call.boxes, call.frames) if on_device else None)
    device = _call_device(call.boxes, call.frames)
    if tracks.state.device != device:
        raise ValueError(f'the track table is on {tracks.state.device}, the call runs on {device}')
    with torch.cuda.device(device):
        slots = _device_slots(track_index, n, device)
        d_fi = call.boxes.device_fi if isinstance(call.boxes, _DeviceBoxes) and call.boxes.device_fi is not None else \
            (call.boxes.host_fi if isinstance(call.boxes, _DeviceBoxes) else call.fi)
        times = _device_times(timestamps, d_fi, n, device)
    return _locate_poses_views(call, model_path, cameras, scale_recovery, targets, per_pose, root_z, coords, sk, False,
                               tracked=(tracks.state, slots, times, prior))[0]


def _tracked_frame_poses(eng, plain: FramePoses, post, reason, coords01, places, scale_recovery, coords, d_targets, per_pose, root_z,
                         n: int, nv: int) -> TrackedFramePoses:
    """The posterior half of locate_tracked_poses_in_frames, enqueued behind the plain half: the same placement, merge and
    covariance launches on the posterior's means and covariances."""
    from metro_pose3d_amd.heads import place_covariances
    from metro_pose3d_amd.inference import posterior_to_metric
    sk = eng.spec.skeleton
    device = post.device
    perm = _upload(np.asarray(sk.permutation, np.int64), device)
    c01 = coords01.clone()
    c01.index_copy_(1, perm, post[..., 2:5].contiguous())
    rel = posterior_to_metric(eng.spec, post, coords01).poses.contiguous() if scale_recovery == 'metro' else None
    poses_v, keypoints_v, z_v, mirror = _place_poses(eng, c01, rel, places, scale_recovery, coords, d_targets, per_pose, root_z)
    poses, keypoints, z_offset, _ = _merge_views(poses_v, keypoints_v, z_v, places, mirror, n, nv, spread=False)
    cov_head = torch.zeros((n * nv, sk.n_head, 6), dtype=torch.float32, device=device)
    cov_head.index_copy_(1, perm, post[..., 5:11].contiguous())
    peak_head = torch.zeros((n * nv, sk.n_head), dtype=torch.float32, device=device)
    peak_head.index_copy_(1, perm, post[..., 1].contiguous())
    cov = place_covariances(cov_head, peak_head, eng.spec, coords, places.reshape(-1) if coords != 'crop' else None, nv)[0]
    posterior = FramePoses(poses, keypoints, z_offset, plain.joint_edges, plain.joint_names)
    return TrackedFramePoses(plain, posterior, cov, post[..., 0].reshape(n, nv, sk.n_out).contiguous(),
                             post[..., 1].reshape(n, nv, sk.n_out).contiguous(), reason.view(n, nv, sk.n_out))


class SkeletonFramePoses(NamedTuple):
    """locate_skeleton_poses_in_frames: `plain` is locate_poses_in_frames' result bit for bit; `selected` the same placement of
    the heat-map modes the person's bone lengths choose; the rest stays per view row ([n, V, ...], V = 1 without views)."""
    plain: FramePoses
    selected: FramePoses
    choice: torch.Tensor         # int32 [n, V, Jout]: the joint's mode in the most probable assignment of the skeleton, -1: none usable
    prob: torch.Tensor           # float32 [n, V, Jout, K]: the marginal probability of every mode under the skeleton
    log_evidence: torch.Tensor   # float32 [n, V, Jout]: ln of the probability the modes give to the bone lengths (<= 0), per component
    log_map: torch.Tensor        # float32 [n, V, Jout]: ln of the probability of the chosen assignment of the joint's component


def locate_skeleton_poses_in_frames(frames, boxes, model_path, cameras, bone_lengths, frame_index=None, k: int = 2, radius: int = 1,
                                    sigma_mm: float = 20.0, sigma_rel: float = 0.0, cov_scale: float = 1.0,
                                    min_length_mm: float = 1.0, scale_recovery: str = 'bone-lengths', root_depth=None,
                                    coords: str = 'camera', precision: Optional[str] = None, check_finite: Optional[bool] = None,
                                    views=None, geometry: str = 'auto', pixel_format: str = 'rgb', color_matrix: str = 'bt601',
                                    crop_dtype: str = 'float32') -> SkeletonFramePoses:
    """locate_poses_in_frames that also chooses among every joint's heat-map modes by the person's bone lengths ->
    SkeletonFramePoses(plain, selected, choice, prob, log_evidence, log_map).  A wrist's heat-map with two peaks (a left / right
    swap, a second person in the crop) has its mean between them, and its heavier peak may be the wrong one; only one of them is a
    forearm's length from the elbow.  From one camera and one frame, without a track, that is what can tell them apart.

    frames, boxes, cameras, frame_index and every keyword from scale_recovery on are locate_poses_in_frames'.  bone_lengths: mm
    over skeleton.edges (the order of head_edges), [E] or [n, E], host values or a float64 CUDA tensor [n, E], contiguous, on the
    call's device (Follower.bone_lengths_for's tensor as it is: never read on the host).  They choose the modes and, under
    scale_recovery 'bone-lengths', also place both poses, so they must then be finite and positive; under 'metro' and
    'true-root-depth' a NaN (or a value <= 0) says that a bone is unknown.  k, radius: the modes (estimate_pose_modes); sigma_mm,
    sigma_rel, cov_scale, min_length_mm: heads.skeleton_mode_params, which says of the defaults that they are design choices.
    One enqueue chain and ONE synchronisation, locate_poses_in_frames' own with the modes and the skeleton bound to the forward
    (Engine.forward_skeleton_modes: the modes launch and one more small launch).  The lengths are repeated per view on the
    device; a flipped view shows every joint where its mirror joint is, so its columns are gathered through
    Skeleton.edge_mirror().  `plain` is locate_poses_in_frames' result, bit for bit.  `selected` is placed by the same
    metro_place_poses and metro_merge_views launches on coords01_sel, the forward's coords01 with the chosen modes' means in
    place of the plain ones (scale_recovery 'metro' roots them as inference.skeleton_to_metric does).  choice, prob and both logs
    stay per view row.
    Limits: it can only choose among the modes heat_modes found; lengths are compared in MeTRo's metric scale (the linear part of
    heatmap_to_metric), which is not the scale bone lengths place the pose in; sharded calls are not served.
    ValueError before any launch for a bad k, radius or option, bone lengths of another shape, dtype or device, and whatever
    locate_poses_in_frames refuses."""
    from metro_pose3d_amd.heads import skeleton_mode_params
    call = _checked_call(frames, boxes, frame_index, coords, views, geometry, precision, check_finite, pixel_format,
                         color_matrix, crop_dtype)
    for name, v, lo, hi in (('k', k, 1, _lib.METRO_MAX_MODES), ('radius', radius, 0, _lib.METRO_MAX_MODE_RADIUS)):
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError(f'{name} must be an int in [{lo}, {hi}], got {v!r}')
    options = dict(sigma_mm=sigma_mm, sigma_rel=sigma_rel, cov_scale=cov_scale, min_length_mm=min_length_mm)
    skeleton_mode_params((1.0, 1.0, 1.0), **options)
    sk = _model_skeleton(model_path)
    n, n_edges = len(call.boxes), len(sk.edges)
    device = _call_device(call.boxes, call.frames)
    if bone_lengths is None:
        raise ValueError(f'bone_lengths is required: mm over the model\'s {n_edges} edges (skeleton.edges), [E] or [n, E]')
    if isinstance(bone_lengths, torch.Tensor) and bone_lengths.is_cuda:
        t = bone_lengths
        if t.dtype != torch.float64 or tuple(t.shape) != (n, n_edges) or not t.is_contiguous() or t.device != device:
            raise ValueError(f'a CUDA tensor as bone_lengths must be a contiguous float64 [{n}, {n_edges}] tensor on the call\'s device '
                             f'(Follower.bone_lengths_for), got {t.dtype} {tuple(t.shape)} on {t.device}')
        place_with = t
    else:
        b = np.asarray(bone_lengths.numpy() if isinstance(bone_lengths, torch.Tensor) else bone_lengths, np.float64)
        if b.shape not in ((n_edges,), (n, n_edges)):
            raise ValueError(f'bone_lengths must be [{n_edges}] or [{n}, {n_edges}] (mm over skeleton.edges), got {b.shape}')
        place_with = np.ascontiguousarray(b)
    placed = scale_recovery == 'bone-lengths'
    targets, per_pose, root_z = _placement_targets(scale_recovery, cameras, n, len(sk.head_edges), place_with if placed else None,
                                                   root_depth, device if isinstance(place_with, torch.Tensor) else None)
    with torch.cuda.device(device):
        rows = place_with if isinstance(place_with, torch.Tensor) else \
            _upload(np.array(np.broadcast_to(place_with, (n, n_edges)), np.float64), device)
    return _locate_poses_views(call, model_path, cameras, scale_recovery, targets, per_pose, root_z, coords, sk, False,
                               skeleton=(rows, k, radius, options))[0]


def _skeleton_frame_poses(eng, plain: FramePoses, sel, choice, prob, info, places, scale_recovery, coords, d_targets, per_pose, root_z,
                          n: int, nv: int) -> SkeletonFramePoses:
    """The selected half of locate_skeleton_poses_in_frames, enqueued behind the plain half: the same placement and merge launches
    on coords01_sel."""
    from metro_pose3d_amd.inference import skeleton_to_metric
    sk = eng.spec.skeleton
    rel = skeleton_to_metric(eng.spec, sel).contiguous() if scale_recovery == 'metro' else None
    poses_v, keypoints_v, z_v, mirror = _place_poses(eng, sel, rel, places, scale_recovery, coords, d_targets, per_pose, root_z)
    poses, keypoints, z_offset, _ = _merge_views(poses_v, keypoints_v, z_v, places, mirror, n, nv, spread=False)
    selected = FramePoses(poses, keypoints, z_offset, plain.joint_edges, plain.joint_names)
    return SkeletonFramePoses(plain, selected, choice.view(n, nv, sk.n_out), prob.view(n, nv, sk.n_out, -1),
                              info[..., 0].reshape(n, nv, sk.n_out).contiguous(), info[..., 1].reshape(n, nv, sk.n_out).contiguous())


# ---- one object per followed stream: the keywords checked once, the table of tracks carried from call to call ----

_FOLLOWER_GIVEN = ('frames', 'boxes', 'model_path', 'cameras', 'frame_index', 'timestamps', 'tracks', 'capacity', 'assignment')


class Follower:
    """A followed stream: follow_poses_in_frames (world=False: one calibrated camera, tracks in its frame or, with
    coords='world', in the world) or follow_world_poses_in_frames (world=True: a calibrated rig) with the model, the
    cameras, the assignment rule and every keyword fixed at construction, and the table of tracks kept between calls.

    Follower(..., world=True, single_view='rays' or 'skip'): follow_rig_poses_in_frames instead, in which a person one camera
    sees keeps feeding its track; `keywords` then also takes ray_depth_sigma_mm.  Without single_view it is what it was.
    Follower(model_path, cameras, world=False, assignment='greedy', capacity=64, **keywords): `keywords` are those of the
    chosen call other than frames, boxes, model_path, cameras, frame_index, timestamps, tracks and capacity; an unknown name
    is a TypeError here, and the values are checked here by the calls' own validators (heads.association_params,
    heads.smoothing_params and, with world=True, heads.matching_params and heads.triangulation_min_det), so a bad keyword
    fails before the first frame.  assignment: 'greedy' or 'optimal', heads.associate_tracks' rule.
    .follow(frames, boxes, frame_index, timestamps) -> FollowedPoses / FollowedWorldPoses of these boxes, continuing
    .tracks (None before the first call: a fresh table of `capacity` slots), which then is the table the call returned.
    .predict(frame_sizes, timestamps, **keywords) -> predict_boxes_in_frames on .tracks with the follower's cameras and
    coordinates.  .reset() drops the table: the next call starts new tracks from id 0.
    Follower(..., world=True, learn_bones=True): every call also learns the bone lengths of the persons it follows, per track
    slot, from their triangulated joints and covariance (one metro_track_bone_lengths launch at the end of the chain, still one
    synchronisation; heads.track_bone_lengths has the estimator, run with its defaults and the follower's sigma_floor_mm and
    cov_scale).  Every output of .follow is what it is without learn_bones, and without it the follower enqueues what it did.
    world=False is refused: lengths learned from poses that bone lengths placed would only echo the table (learning under
    'true-root-depth' is left out).  .bones is the BoneTable (None before the first call); .bone_lengths(fallback=None) ->
    heads.BoneLengths of every slot, one read-out launch; .bone_lengths_for(track_index, fallback) -> float64 [n, E] on the
    device, one row per entry of an int32 CUDA tensor of slots such as PredictedBoxes.track_index: the slot's learned lengths,
    `fallback` (required: [E] finite and positive mm) for -1, for a slot outside the table and for every edge not yet known
    -- so every value is finite and positive and the tensor goes straight into locate_poses_in_frames(bone_lengths=...): a rig
    that has seen a person lets any one camera place that person with their own skeleton, with no host round trip.  Neither
    synchronises.  .reset() also drops the bone table."""

    def __init__(self, model_path, cameras, world: bool = False, assignment: str = 'greedy', capacity: int = 64,
                 single_view: Optional[str] = None, learn_bones: bool = False, **keywords):
        import inspect
        if not isinstance(world, (bool, np.bool_)):
            raise ValueError(f'world must be True or False, got {world!r}')
        if not isinstance(learn_bones, (bool, np.bool_)):
            raise ValueError(f'learn_bones must be True or False, got {learn_bones!r}')
        if learn_bones and not world:
            raise ValueError('learn_bones needs world=True: bone lengths are learned from triangulated poses; poses that bone '
                             'lengths placed would only echo the table')
        if single_view is not None and not world:
            raise ValueError('single_view belongs to a calibrated rig: it needs world=True')
        call = follow_poses_in_frames if not world else follow_world_poses_in_frames if single_view is None else follow_rig_poses_in_frames
        params = inspect.signature(call).parameters
        defaults = {k: p.default for k, p in params.items() if k not in _FOLLOWER_GIVEN + ('single_view',)}
        unknown = [k for k in keywords if k not in defaults]
        if unknown:
            raise TypeError(f"Follower(world={bool(world)}) got an unexpected keyword {unknown[0]!r}: it takes "
                            f"{', '.join(defaults)}")
        kw = dict(defaults, **keywords)
        new_track_table(capacity, 1, 'cpu')                 # the capacity check
        if world:                                           # the option groups, checked here, once: follow() hands them on
            self._groups = _world_groups(kw, assignment, 'skip' if single_view is None else single_view)
            if cameras is None:
                raise ValueError('cameras: following in the world needs the calibrated cameras of the rig')
        else:
            self._groups = _camera_groups(kw, assignment)
        self.model_path, self.cameras, self.world = model_path, cameras, bool(world)
        self.assignment, self.capacity, self.keywords, self.single_view = assignment, int(capacity), kw, single_view
        self.tracks: Optional[TrackTable] = None
        self.learn_bones = bool(learn_bones)
        self.bones: Optional[BoneTable] = None

    def follow(self, frames, boxes, frame_index, timestamps):
        given = (frames, boxes, self.model_path, self.cameras, frame_index, timestamps, self.tracks, self.capacity)
        if self.world:
            bones = (True if self.bones is None else self.bones) if self.learn_bones else None
            out, extra, self.bones = _follow_world(*given, *self._groups, bones)
            if self.single_view is not None:
                out = _rig_poses(out, extra)
        else:
            out = _follow_poses(*given, *self._groups)
        self.tracks = out.tracks
        return out

    def predict(self, frame_sizes, timestamps, **keywords) -> PredictedBoxes:
        if self.tracks is None:
            raise ValueError('Follower.predict: no table of tracks yet (call follow first)')
        if 'coords' in keywords:
            raise TypeError("Follower.predict: coords is the follower's own")
        coords = 'world' if self.world else self.keywords['coords']
        return predict_boxes_in_frames(self.tracks, self.cameras, frame_sizes, timestamps, coords=coords, **keywords)

    def locate(self, frames, boxes, track_index, frame_index, timestamps, **keywords) -> TrackedFramePoses:
        """locate_tracked_poses_in_frames on .tracks with the follower's model, cameras, table coordinates, accel_psd, max_age_s
        and locate keywords (scale_recovery, bone_lengths, root_depth, coords, views, ...); `keywords` override those and take
        depth, near_mm, sigma_floor_mm and cov_scale.  boxes, frame_index and track_index may be .predict's CUDA tensors."""
        if self.tracks is None:
            raise ValueError('Follower.locate: no table of tracks yet (call follow first)')
        if 'table_coords' in keywords:
            raise TypeError("Follower.locate: table_coords is the follower's own")
        table_coords = 'world' if self.world else self.keywords['coords']
        if table_coords not in ('camera', 'world'):
            raise ValueError(f"Follower.locate: the follower's tracks live in {table_coords!r} coordinates; a track prior needs a "
                             "table in 'camera' or 'world' coordinates")
        import inspect
        params = inspect.signature(locate_tracked_poses_in_frames).parameters
        kw = {k: self.keywords[k] for k in ('accel_psd', 'max_age_s') + _LOCATE_OPTIONS if k in self.keywords and k in params}
        unknown = [k for k in keywords if k not in params or k in _FOLLOWER_GIVEN + ('track_index',)]
        if unknown:
            raise TypeError(f'Follower.locate got an unexpected keyword {unknown[0]!r}')
        kw.update(keywords)
        return locate_tracked_poses_in_frames(frames, boxes, self.model_path, self.cameras, self.tracks, track_index, frame_index,
                                              timestamps, table_coords=table_coords, **kw)

    def locate_skeleton(self, frames, boxes, track_index, frame_index, fallback, **keywords) -> SkeletonFramePoses:
        """locate_skeleton_poses_in_frames on .bone_lengths_for(track_index, fallback): every box's heat-map modes chosen among,
        and both poses placed, by the followed person's own learned skeleton (`fallback` [E] mm for -1, for a slot outside the
        table and for every edge not yet known).  Needs learn_bones=True; track_index: an int32 CUDA tensor of slots such as
        PredictedBoxes.track_index; `keywords` are that call's (k, radius, sigma_mm, ..., scale_recovery, coords, views, ...).  No
        host round trip: the lengths are never read on the host."""
        if 'bone_lengths' in keywords:
            raise TypeError("Follower.locate_skeleton: bone_lengths are the follower's own")
        lengths = self.bone_lengths_for(track_index, fallback)
        return locate_skeleton_poses_in_frames(frames, boxes, self.model_path, self.cameras, lengths, frame_index, **keywords)

    def _bone_read_out(self, fallback, required: bool):
        from metro_pose3d_amd.heads import bone_fallback, track_bone_lengths
        bone_fallback(fallback, None, required)
        if not self.learn_bones:
            raise ValueError('this follower learns no bone lengths (learn_bones=True)')
        sk = _model_skeleton(self.model_path)
        fallback = bone_fallback(fallback, len(sk.edges), required)
        if self.bones is None or self.tracks is None:
            raise ValueError('no bone table yet (call follow first)')
        with torch.cuda.device(self.bones.stats.device):
            return track_bone_lengths(None, None, None, None, self.tracks.ids, self.bones.stats, self.bones.ids, sk.edges,
                                      sk.edge_mirror(), fallback, sigma_floor_mm=self.keywords['sigma_floor_mm'],
                                      cov_scale=self.keywords['cov_scale'])

    def bone_lengths(self, fallback=None):
        return self._bone_read_out(fallback, False)

    def bone_lengths_for(self, track_index, fallback) -> torch.Tensor:
        from metro_pose3d_amd.heads import bone_fallback
        bone_fallback(fallback, None, True)
        if (not isinstance(track_index, torch.Tensor) or not track_index.is_cuda or track_index.dtype != torch.int32
                or track_index.dim() != 1):
            raise ValueError('track_index must be an int32 CUDA tensor [n] of track slots (PredictedBoxes.track_index), got '
                             f'{getattr(track_index, "dtype", type(track_index))} {tuple(getattr(track_index, "shape", ()))}')
        table = self._bone_read_out(fallback, True).lengths               # unknown edges already hold the fallback
        if track_index.device != table.device:
            raise ValueError(f'track_index is on {track_index.device}, the bone table on {table.device}')
        # row T of the padded table is the fallback itself (an unknown edge of ANY slot holds it): -1 and slots outside go there
        n_tracks = table.shape[0]
        slot = track_index.to(torch.int64)
        slot = torch.where((slot >= 0) & (slot < n_tracks), slot, torch.full_like(slot, n_tracks))
        row = _upload(bone_fallback(fallback, table.shape[1], True), table.device)
        return torch.cat([table, row[None]], 0).index_select(0, slot).contiguous()

    def reset(self):
        self.tracks = None
        self.bones = None
