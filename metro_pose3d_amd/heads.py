"""Alternative decode heads of the reference, the step AFTER the hot path, on the GPU
through the C ABI (csrc/heads.hip).  Names and argument meaning follow the reference:

  coords01_from_logits      net_output_to_heatmap_and_coords          src/model/volumetric.py:227-235
  moments_from_logits       the same + covariance and peak of every joint's softmax volume (the graph's unused by-product
                            `heatmap_pred_z`, volumetric.py:165, is a marginal of it)
  place_covariances         Cov01 -> mm^2 in output order and crop / camera / world axes, views averaged
  triangulate_joints        world joints of persons seen by several calibrated cameras: the point nearest to the rays of
                            their crops, uniform or heat-map-covariance weights (nothing in the reference: one camera each)
  view_affinity             how close the per-joint rays of every two boxes of several cameras pass: the cost matrix of
                            cross-view association (nothing in the reference: one camera each)
  view_affinity_steps       the same gated by time step: boxes of different exposures of the rig are never compared
  cluster_views             constrained complete-linkage clustering of that matrix: person_index and the CSR grouping
                            triangulate_joints reads, all on the device
  person_steps              the time step of every person cluster_views found and the time-step CSR associate_tracks reads,
                            on the device
  associate_tracks          which box of a video continues which track: greedy or optimal assignment on predicted poses, births and the
                            CSR grouping smooth_tracks reads, one workgroup
  predict_boxes             next-frame person boxes from the track table: the filter's prediction of every live track through
                            the frames' calibrated cameras, compacted on the device and fused with a detector's boxes
  track_prior_params        the options of the track-predicted heat-map prior (Engine.forward_track_posterior,
                            frames.locate_tracked_poses_in_frames), checked
  fusion_params             the options of the view fusion (Engine.forward_view_fusion, frames.fuse_poses_in_frames), checked:
                            Fusion, whose record() is the MetroViewFusion metro_plan_bind_view_fusion copies
  skeleton_mode_params      the options of the choice among heat-map modes by bone lengths (Engine.forward_skeleton_modes,
                            estimate_pose_skeleton), checked: the MetroSkeletonModes metro_plan_bind_skeleton_modes copies
  smooth_tracks             poses of tracked persons over time: constant-velocity Kalman filter / RTS smoother per track and
                            joint, each row weighted by its heat-map covariance (nothing in the reference: one image each)
  track_bone_lengths        the bone lengths of followed persons, learned per track slot from their triangulated joints: a
                            covariance-weighted, noise-debiased, gated mean per skeleton edge (nothing in the reference: its
                            tables come from its training data)
  backproject_bone_lengths  scale_recovery 'bone-lengths' / '-true'   volumetric.py:171-191,
                            optimize_z_offset_by_bones(_tensor)       src/model/bone_length_based_backproj.py:15-62
  backproject_root_depth    scale_recovery 'true-root-depth'          volumetric.py:192-199
  heatmap_to_25d            crop pixels + z * box_size                volumetric.py:298-300
  to_orig_cam               rotation + mirror on det(R) <= 0          volumetric.py:277-281

MeTRo's own output (`scale_recovery == 'metro'`, volumetric.py:200-201) is `Engine.forward` / `estimate_pose`.
There is no CPU fallback: without the HIP library these raise MetroError."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from metro_pose3d_amd import _lib
from metro_pose3d_amd._lib import check
from metro_pose3d_amd.spec import ModelSpec


def _p(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream(dev) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


_TABLES = {}                       # (device, dtype, shape, bytes) -> the device copy of a small constant table
_TABLES_MAX = 64


def _table(values, dtype, dev) -> torch.Tensor:
    """A small constant table (a skeleton's mirror joints or edges, an index pattern) on the device.  Uploaded once per device
    with a BLOCKING copy -- complete before any stream can read it, whichever stream is current now or at a later call -- and
    kept: every later call uses the copy, launches no transfer and does not wait for its stream (a pageable upload per call
    made the wrappers synchronise; tests/test_gpu_streams.py).  At most _TABLES_MAX tables are kept (the tables of a few
    skeletons; callers may pass their own edges and mirror mappings): past that a table is uploaded, blocking, for the call
    alone.  Nothing is ever dropped from the cache: a launch queued on some stream may still read it."""
    a = np.ascontiguousarray(np.asarray(values, dtype))
    key = (str(dev), a.dtype.str, a.shape, a.tobytes())
    t = _TABLES.get(key)
    if t is None:
        t = torch.from_numpy(a).to(dev)
        if len(_TABLES) < _TABLES_MAX:
            _TABLES[key] = t
    return t


def _f32(x, dev, shape_tail) -> torch.Tensor:
    t = torch.as_tensor(x, dtype=torch.float32, device=dev).contiguous()
    if tuple(t.shape[1:]) != tuple(shape_tail):
        raise ValueError(f'expected [N,{",".join(map(str, shape_tail))}], got {tuple(t.shape)}')
    return t


def coords01_from_logits(logits: torch.Tensor, spec: ModelSpec, precise: int = 1) -> torch.Tensor:
    """fp32 (precise 0/1) or fp64 (precise 2) NHWC logits [N,S,S,D*J] -> soft-argmax coords in [0,1] [N,J,3]."""
    lib = _lib.load()
    if logits.dim() != 4 or logits.shape[1] != spec.heatmap_side or logits.shape[3] != spec.n_head_channels:
        raise ValueError(f'logits must be [N,{spec.heatmap_side},{spec.heatmap_side},{spec.n_head_channels}]')
    logits = logits.to(torch.float64 if precise == 2 else torch.float32).contiguous()
    n = logits.shape[0]
    cs = spec.to_c(int(precise))
    scratch = torch.empty(lib.metro_softargmax_scratch_bytes(n, spec.heatmap_side, spec.skeleton.n_head),
                          dtype=torch.uint8, device=logits.device)
    out = torch.empty((n, spec.skeleton.n_head, 3), dtype=torch.float32, device=logits.device)
    check(lib.metro_softargmax01(_p(logits), n, C.byref(cs), int(precise), _p(scratch), _p(out), _stream(logits.device)),
          'metro_softargmax01')
    return out


def cov6_to_3x3(cov6: torch.Tensor) -> torch.Tensor:
    """[..., 6] (xx, yy, zz, xy, xz, yz) -> symmetric [..., 3, 3]."""
    idx = _table([0, 3, 4, 3, 1, 5, 4, 5, 2], np.int64, cov6.device)
    return cov6[..., idx].reshape(*cov6.shape[:-1], 3, 3)


def moments_from_logits(logits: torch.Tensor, spec: ModelSpec, precise: int = 1):
    """fp32 (precise 0/1) or fp64 (precise 2) NHWC logits [N,S,S,D*J] -> (coords01 [N,J,3], cov01 [N,J,3,3], peak [N,J]), head
    order.  Per joint, with p its softmax over the S*S*D voxels and c their linspace(0,1,.) coordinates: coords01 = sum p c,
    cov01 = sum p (c - coords01)(c - coords01)^T, peak = max p.  The covariance of the joint's OWN heat-map in the crop's
    virtual-camera axes (units of coords01), not of the root-relative difference."""
    lib = _lib.load()
    if logits.dim() != 4 or logits.shape[1] != spec.heatmap_side or logits.shape[3] != spec.n_head_channels:
        raise ValueError(f'logits must be [N,{spec.heatmap_side},{spec.heatmap_side},{spec.n_head_channels}]')
    if precise not in (0, 1, 2):
        raise ValueError(f'precise must be 0, 1 or 2, got {precise!r}')
    logits = logits.to(torch.float64 if precise == 2 else torch.float32).contiguous()
    n, nj, dev = logits.shape[0], spec.skeleton.n_head, logits.device
    cs = spec.to_c(int(precise))
    scratch = torch.empty(lib.metro_softargmax_scratch_bytes(n, spec.heatmap_side, nj), dtype=torch.uint8, device=dev)
    mscratch = torch.empty(lib.metro_moments_scratch_bytes(C.byref(cs), n), dtype=torch.uint8, device=dev)
    c01 = torch.empty((n, nj, 3), dtype=torch.float32, device=dev)
    cov = torch.empty((n, nj, 6), dtype=torch.float32, device=dev)
    peak = torch.empty((n, nj), dtype=torch.float32, device=dev)
    check(lib.metro_softargmax01_moments(_p(logits), n, C.byref(cs), int(precise), _p(scratch), _p(mscratch), _p(c01), _p(cov),
                                         _p(peak), _stream(dev)), 'metro_softargmax01_moments')
    return c01, cov6_to_3x3(cov), peak


def _heat_logits(logits: torch.Tensor, spec: ModelSpec, precise: int) -> torch.Tensor:
    if logits.dim() != 4 or logits.shape[0] < 1 or tuple(logits.shape[1:]) != (spec.heatmap_side, spec.heatmap_side, spec.n_head_channels):
        raise ValueError(f'logits must be [N,{spec.heatmap_side},{spec.heatmap_side},{spec.n_head_channels}]')
    if precise not in (0, 1, 2):
        raise ValueError(f'precise must be 0, 1 or 2, got {precise!r}')
    return logits.to(torch.float64 if precise == 2 else torch.float32).contiguous()


def marginals_from_logits(logits: torch.Tensor, spec: ModelSpec, precise: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 (precise 0/1) or fp64 (precise 2) NHWC logits [N,S,S,D*J] -> (xy [N,Jout,S,S], z [N,Jout,D]): the heat-map marginals
    of a forward with bound heat-map buffers (metro_plan_bind_heatmaps), from the caller's logits, output joint order."""
    lib = _lib.load()
    logits = _heat_logits(logits, spec, precise)
    n, nj, side, dev = logits.shape[0], spec.skeleton.n_out, spec.heatmap_side, logits.device
    cs = spec.to_c(int(precise))
    scratch = torch.empty(lib.metro_heat_marginals_scratch_bytes(C.byref(cs), n), dtype=torch.uint8, device=dev)
    xy = torch.empty((n, nj, side, side), dtype=torch.float32, device=dev)
    z = torch.empty((n, nj, spec.depth), dtype=torch.float32, device=dev)
    check(lib.metro_heat_marginals(_p(logits), n, C.byref(cs), int(precise), _p(scratch), _p(xy), _p(z), _stream(dev)),
          'metro_heat_marginals')
    return xy, z


def modes_from_logits(logits: torch.Tensor, spec: ModelSpec, k: int = 2, radius: int = 1,
                      precise: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """Logits as above -> (voxel int32 [N,Jout,k], stats [N,Jout,k,11]: mass, peak, coords01, cov01): the heat-map modes of a
    forward with bound mode buffers (metro_plan_bind_modes), from the caller's logits, output joint order."""
    lib = _lib.load()
    logits = _heat_logits(logits, spec, precise)
    for name, v, lo, hi in (('k', k, 1, _lib.METRO_MAX_MODES), ('radius', radius, 0, _lib.METRO_MAX_MODE_RADIUS)):
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError(f'{name} must be an int in [{lo}, {hi}], got {v!r}')
    n, nj, dev = logits.shape[0], spec.skeleton.n_out, logits.device
    cs = spec.to_c(int(precise))
    voxel = torch.empty((n, nj, k), dtype=torch.int32, device=dev)
    stats = torch.empty((n, nj, k, 11), dtype=torch.float32, device=dev)
    check(lib.metro_heat_modes(_p(logits), n, C.byref(cs), int(precise), k, radius, _p(voxel), _p(stats), _stream(dev)),
          'metro_heat_modes')
    return voxel, stats


def posterior_from_logits(logits: torch.Tensor, prior: torch.Tensor, spec: ModelSpec, precise: int = 1) -> torch.Tensor:
    """Logits as above and prior rows [N,Jout,9] (mu, precision) -> post [N,Jout,11]: the heat-map posterior of a forward with
    bound prior buffers (metro_plan_bind_prior), from the caller's logits, output joint order."""
    lib = _lib.load()
    logits = _heat_logits(logits, spec, precise)
    n, nj, dev = logits.shape[0], spec.skeleton.n_out, logits.device
    if tuple(prior.shape) != (n, nj, 9):
        raise ValueError(f'prior must be [{n},{nj},9], got {tuple(prior.shape)}')
    prior = prior.to(device=dev, dtype=torch.float32).contiguous()
    cs = spec.to_c(int(precise))
    post = torch.empty((n, nj, 11), dtype=torch.float32, device=dev)
    check(lib.metro_heat_posterior(_p(logits), n, C.byref(cs), int(precise), _p(prior), _p(post), _stream(dev)),
          'metro_heat_posterior')
    return post


_COORDS = {'crop': _lib.METRO_COORDS_CROP, 'camera': _lib.METRO_COORDS_CAMERA, 'world': _lib.METRO_COORDS_WORLD}


def place_covariances(cov01: torch.Tensor, peak: torch.Tensor, spec: ModelSpec, coords: str = 'crop',
                      records: Optional[torch.Tensor] = None, n_views: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """cov01 [R,J_head,6] + peak [R,J_head] of R = n * n_views crops (box-major rows) -> (covariance [n,Jout,3,3] mm^2,
    peak [n,Jout]) in output joint order: diag(s) Cov01 diag(s) with s = (lrc box / proc_side, the same, box) -- the linear part
    of heatmap_to_metric -- then, for coords 'camera' / 'world', R Cov R^T with the rotation of each row's MetroPlacement in
    `records` (a uint8 device tensor of R records), mirror joints swapped where det R <= 0; the mean over the views."""
    lib = _lib.load()
    if coords not in _COORDS:
        raise ValueError(f"coords must be 'crop', 'camera' or 'world', got {coords!r}")
    nj = spec.skeleton.n_head
    if cov01.dim() != 3 or tuple(cov01.shape[1:]) != (nj, 6) or tuple(peak.shape) != tuple(cov01.shape[:2]):
        raise ValueError(f'cov01 must be [R,{nj},6] and peak [R,{nj}], got {tuple(cov01.shape)} and {tuple(peak.shape)}')
    n_views = int(n_views)
    if n_views < 1 or n_views > _lib.METRO_MAX_VIEWS or cov01.shape[0] % n_views:
        raise ValueError(f'{cov01.shape[0]} rows are not a whole number of boxes of {n_views} views (1 to {_lib.METRO_MAX_VIEWS})')
    if coords != 'crop':
        need = cov01.shape[0] * C.sizeof(_lib.MetroPlacement)
        if records is None or records.dtype != torch.uint8 or records.numel() != need:
            raise ValueError(f"coords {coords!r} needs `records`: a uint8 tensor of {cov01.shape[0]} MetroPlacement ({need} bytes)")
    dev = cov01.device
    cov01 = cov01.to(torch.float32).contiguous()
    peak = peak.to(torch.float32).contiguous()
    n = cov01.shape[0] // n_views
    cs = spec.to_c(1)
    mirror = _table(spec.skeleton.out_mirror, np.int32, dev) if coords != 'crop' else None
    out = torch.empty((n, spec.skeleton.n_out, 9), dtype=torch.float32, device=dev)
    pk = torch.empty((n, spec.skeleton.n_out), dtype=torch.float32, device=dev)
    check(lib.metro_place_covariances(_p(cov01), _p(peak), _p(records if coords != 'crop' else None), n, n_views, C.byref(cs),
                                      _p(mirror), _COORDS[coords], _p(out), _p(pk), _stream(dev)), 'metro_place_covariances')
    return out.view(n, spec.skeleton.n_out, 3, 3), pk


TRI_WEIGHTS = {'uniform': _lib.METRO_TRI_UNIFORM, 'covariance': _lib.METRO_TRI_COVARIANCE}


def triangulation_min_det(weights, min_angle_deg) -> float:
    """Checks `weights` and `min_angle_deg` of the triangulation calls; returns min_det = sin^2(min_angle) / 4, the determinant
    of the normalised system of two rays at that angle (metro_triangulate_joints)."""
    if not isinstance(weights, str) or weights not in TRI_WEIGHTS:
        raise ValueError(f"weights must be 'uniform' or 'covariance', got {weights!r}")
    if (isinstance(min_angle_deg, (bool, np.bool_)) or not isinstance(min_angle_deg, (int, float, np.integer, np.floating))
            or not 0 < min_angle_deg <= 90):
        raise ValueError(f'min_angle_deg must lie in (0, 90] degrees, got {min_angle_deg!r}')
    return float(np.sin(np.radians(float(min_angle_deg))) ** 2 / 4.0)


class Triangulation(NamedTuple):
    """The triangulation keywords of the frames calls, checked once, where the group is built (`checked`)."""
    weights: str
    min_angle_deg: float

    @classmethod
    def checked(cls, weights, min_angle_deg) -> 'Triangulation':
        triangulation_min_det(weights, min_angle_deg)
        return cls(weights, min_angle_deg)


def _i32(x, dev) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        return x.to(device=dev, dtype=torch.int32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(np.int32))).to(dev)


def triangulate_joints(coords01: torch.Tensor, cov01: Optional[torch.Tensor], places: torch.Tensor, rows, starts,
                       spec: ModelSpec, weights: str = 'covariance', min_angle_deg: float = 2.0,
                       return_covariance: bool = False):
    """World joints of P persons from the rays of their crop rows, one metro_triangulate_joints launch.
    coords01 [m,J_head,3] and (weights 'covariance') cov01 [m,J_head,6] as the forward writes them, `places` a uint8 device
    tensor of m MetroPlacement records (the crops' virtual cameras), person p owning the crop rows rows[starts[p]:starts[p+1]]
    (int arrays or tensors; starts [P+1], from 0 to len(rows), a group may be empty).  -> (points [P,Jout,3] world mm,
    n_rays int32 [P,Jout], residual [P,Jout] mm) on the device.  'uniform': the point nearest to the rays; 'covariance': a
    second solve that weights each ray by 1 / (sigma^2 z^2), its heat-map's variance carried to the joint's depth.  A joint
    seen by fewer than two rays, or whose rays are within min_angle_deg of parallel (det of the normalised system below
    sin^2(min_angle) / 4), is NaN; n_rays still counts its usable rays.
    return_covariance=True: one metro_triangulate_joints_cov launch instead, the same three outputs bit for bit and a fourth,
    covariance [P,Jout,9] mm^2 (row-major symmetric 3x3, what smooth_tracks and associate_tracks read): the inverse of the
    final solve's system, 'covariance': (sum w (I - d d^T))^-1, w being an inverse variance; 'uniform':
    s^2 (sum (I - d d^T))^-1 with s^2 = sum |p|^2 / (2 k - 3) from the distances of the point to its k rays; NaN where the
    joint is."""
    min_det = triangulation_min_det(weights, min_angle_deg)
    nj, n_out = spec.skeleton.n_head, spec.skeleton.n_out
    if coords01.dim() != 3 or tuple(coords01.shape[1:]) != (nj, 3):
        raise ValueError(f'coords01 must be [m,{nj},3], got {tuple(coords01.shape)}')
    m = coords01.shape[0]
    if weights == 'covariance' and (cov01 is None or tuple(cov01.shape) != (m, nj, 6)):
        raise ValueError(f"weights='covariance' needs cov01 [{m},{nj},6], got {None if cov01 is None else tuple(cov01.shape)}")
    need = m * C.sizeof(_lib.MetroPlacement)
    if not isinstance(places, torch.Tensor) or places.dtype != torch.uint8 or places.numel() != need:
        raise ValueError(f'places must be a uint8 tensor of {m} MetroPlacement records ({need} bytes)')
    dev = coords01.device
    rows, starts = _i32(rows, dev).reshape(-1), _i32(starts, dev).reshape(-1)
    if starts.numel() < 1:
        raise ValueError('starts must hold P + 1 offsets (P >= 0)')
    n_persons = starts.numel() - 1
    lib = _lib.load()
    coords01, places = coords01.to(torch.float32).contiguous(), places.contiguous()
    cov01 = cov01.to(torch.float32).contiguous() if weights == 'covariance' else None
    points = torch.empty((n_persons, n_out, 3), dtype=torch.float32, device=dev)
    n_rays = torch.empty((n_persons, n_out), dtype=torch.int32, device=dev)
    residual = torch.empty((n_persons, n_out), dtype=torch.float32, device=dev)
    out = (points, n_rays, residual)
    if return_covariance:
        out += (torch.empty((n_persons, n_out, 9), dtype=torch.float32, device=dev),)
    if n_persons == 0:
        return out
    cs = spec.to_c(1)
    mirror = _table(spec.skeleton.out_mirror, np.int32, dev)
    entry = 'metro_triangulate_joints_cov' if return_covariance else 'metro_triangulate_joints'
    check(getattr(lib, entry)(_p(coords01), _p(cov01), _p(places), m, _p(rows), rows.numel(), _p(starts), n_persons, C.byref(cs),
                              _p(mirror), TRI_WEIGHTS[weights], min_det, *(_p(t) for t in out), _stream(dev)), entry)
    return out


MATCH_MAX_BOXES = _lib.METRO_MATCH_MAX_BOXES


def _is_number(v) -> bool:
    return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating))


def matching_params(clip_mm, min_joints, *max_cost_mm):
    """Checks `clip_mm`, `min_joints` (None, or an integer >= 1) and, if given, `max_cost_mm` of the matching calls."""
    for name, v in (('clip_mm', clip_mm),) + tuple(('max_cost_mm', v) for v in max_cost_mm):
        if not _is_number(v) or not np.isfinite(v) or not v > 0:
            raise ValueError(f'{name} must be a finite number > 0 (mm), got {v!r}')
    if min_joints is not None and (isinstance(min_joints, (bool, np.bool_)) or not isinstance(min_joints, (int, np.integer))
                                   or min_joints < 1):
        raise ValueError(f'min_joints must be None or an integer >= 1, got {min_joints!r}')


class Matching(NamedTuple):
    """The cross-view matching keywords of the frames calls, checked once, where the group is built (`checked`)."""
    max_cost_mm: float
    clip_mm: float
    min_joints: Optional[int]

    @classmethod
    def checked(cls, max_cost_mm, clip_mm, min_joints) -> 'Matching':
        matching_params(clip_mm, min_joints, max_cost_mm)
        return cls(float(max_cost_mm), float(clip_mm), None if min_joints is None else int(min_joints))


def _check_n_views(n_views, rows: int) -> int:
    if isinstance(n_views, (bool, np.bool_)) or not isinstance(n_views, (int, np.integer)) or not 1 <= n_views <= _lib.METRO_MAX_VIEWS:
        raise ValueError(f'n_views must be an integer from 1 to {_lib.METRO_MAX_VIEWS}, got {n_views!r}')
    if rows % int(n_views):
        raise ValueError(f'{rows} rows are not a whole number of boxes of {n_views} views')
    return int(n_views)


def _checked_crop_rows(coords01, cov01, places, spec, n_views, weights):
    """What view_affinity* and person_rays check alike of the m = n * n_views crop rows -> (m, n_views, n)."""
    nj = spec.skeleton.n_head
    if not isinstance(coords01, torch.Tensor) or coords01.dim() != 3 or tuple(coords01.shape[1:]) != (nj, 3):
        raise ValueError(f'coords01 must be a tensor [m,{nj},3], got {tuple(getattr(coords01, "shape", ()))}')
    m = coords01.shape[0]
    n_views = _check_n_views(n_views, m)
    if m // n_views > MATCH_MAX_BOXES:
        raise ValueError(f'{m // n_views} boxes: matching takes at most {MATCH_MAX_BOXES}')
    if weights == 'covariance' and (cov01 is None or tuple(cov01.shape) != (m, nj, 6)):
        raise ValueError(f"weights='covariance' needs cov01 [{m},{nj},6], got {None if cov01 is None else tuple(cov01.shape)}")
    need = m * C.sizeof(_lib.MetroPlacement)
    if not isinstance(places, torch.Tensor) or places.dtype != torch.uint8 or places.numel() != need:
        raise ValueError(f'places must be a uint8 tensor of {m} MetroPlacement records ({need} bytes)')
    return m, n_views, m // n_views


def view_affinity(coords01: torch.Tensor, cov01: Optional[torch.Tensor], places: torch.Tensor, frame_index, spec: ModelSpec,
                  n_views: int = 1, weights: str = 'covariance', min_angle_deg: float = 2.0, clip_mm: float = 500.0,
                  min_joints: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """How close the per-joint rays of every two boxes pass, one metro_view_affinity launch: the cost of calling two boxes
    of different cameras the same person.  coords01 [m,J_head,3], cov01 [m,J_head,6] (weights 'covariance') and `places`
    (m MetroPlacement records, uint8) as triangulate_joints reads them, m = n * n_views crop rows, box-major; frame_index [n]
    (ints or a tensor): the frame (camera) of each box.  -> (cost float32 [n,n] mm, n_pairs int32 [n,n]) on the device.
    Per pair of boxes, every (view, output joint) gives one pair of rays -- triangulate_joints' rays, the mirror joint for a
    flipped view -- and the distance at which their lines pass; pairs within min_angle_deg of parallel are left out, pairs
    that meet behind a camera count with clip_mm, every distance is capped at clip_mm.  cost is the RMS of these distances,
    each weighted ('covariance') by 1 / (sigma_a^2 t_a^2 + sigma_b^2 t_b^2), the heat-map variances carried to where the rays
    pass.  +inf on the diagonal, for two boxes on one frame (a person appears once per camera) and where fewer than
    min_joints * n_views ray pairs count (min_joints None: (Jout + 1) // 2).  At most 128 boxes."""
    return view_affinity_steps(coords01, cov01, places, frame_index, None, spec, n_views, weights, min_angle_deg, clip_mm, min_joints)


def view_affinity_steps(coords01: torch.Tensor, cov01: Optional[torch.Tensor], places: torch.Tensor, frame_index, step_index,
                        spec: ModelSpec, n_views: int = 1, weights: str = 'covariance', min_angle_deg: float = 2.0,
                        clip_mm: float = 500.0, min_joints: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """view_affinity gated by time step, one metro_view_affinity_steps launch.  step_index [n] (ints or a tensor): the time step
    of each box, one exposure of the rig; two boxes of different steps cost +inf with n_pairs 0, as two boxes of one frame do;
    every other entry has view_affinity's bits.  step_index None is view_affinity.  (A function of its own: view_affinity's
    parameter list is pinned.)"""
    triangulation_min_det(weights, min_angle_deg)
    matching_params(clip_mm, min_joints)
    m, n_views, n = _checked_crop_rows(coords01, cov01, places, spec, n_views, weights)
    n_out = spec.skeleton.n_out
    if min_joints is None:
        min_joints = (n_out + 1) // 2
    if min_joints > n_out:
        raise ValueError(f'min_joints must be at most the {n_out} output joints, got {min_joints!r}')
    for name, index in (('frame_index', frame_index),) + ((('step_index', step_index),) if step_index is not None else ()):
        size = int(index.numel() if isinstance(index, torch.Tensor) else np.asarray(index).size)
        if size != n:
            raise ValueError(f'{name} must hold one value per box ({n}), got {size}')
    dev = coords01.device
    cost = torch.empty((n, n), dtype=torch.float32, device=dev)
    n_pairs = torch.empty((n, n), dtype=torch.int32, device=dev)
    if n == 0:
        return cost, n_pairs
    lib = _lib.load()
    fi = _i32(frame_index, dev).reshape(-1)
    coords01, places = coords01.to(torch.float32).contiguous(), places.contiguous()
    cov01 = cov01.to(torch.float32).contiguous() if weights == 'covariance' else None
    cs = spec.to_c(1)
    mirror = _table(spec.skeleton.out_mirror, np.int32, dev)
    min_sin2 = float(np.sin(np.radians(float(min_angle_deg))) ** 2)
    si = _i32(step_index, dev).reshape(-1) if step_index is not None else None
    entry, steps = ('metro_view_affinity', ()) if si is None else ('metro_view_affinity_steps', (_p(si),))
    check(getattr(lib, entry)(_p(coords01), _p(cov01), _p(places), C.byref(cs), _p(mirror), _p(fi), *steps, n, n_views,
                              TRI_WEIGHTS[weights], min_sin2, float(clip_mm), int(min_joints) * n_views, _p(cost), _p(n_pairs),
                              _stream(dev)), entry)
    return cost, n_pairs


def cluster_views(cost: torch.Tensor, max_cost_mm: float, n_views: int = 1):
    """Boxes -> persons by constrained complete-linkage clustering of view_affinity's cost, one metro_cluster_views launch (one
    workgroup, the matrix in LDS).  cost [n,n] on the device is read as max(cost, cost^T) with NaN as +inf.  Every box starts
    as its own cluster; the two clusters with the smallest cost merge (ties: the lowest box index of the first, then of the
    second) while that cost is < max_cost_mm, the cost between clusters being the LARGEST cost between their boxes: every two
    boxes of a person agree, and since two boxes of one frame cost +inf a person never gets two boxes of one camera.
    -> (person_index int32 [n], persons numbered by their lowest box; n_persons int32 [1]; rows int32 [n * n_views] and
    starts int32 [n + 1]: the CSR grouping triangulate_joints reads, with n as its person count), all on the device.  A person
    with several boxes owns the crop rows i * n_views + v of its boxes in ascending order; a person with one box, and the
    persons >= n_persons, have empty groups; rows past starts[n] are -1.  At most 128 boxes."""
    if not _is_number(max_cost_mm) or not max_cost_mm > 0:
        raise ValueError(f'max_cost_mm must be a number > 0 (mm), got {max_cost_mm!r}')
    if not isinstance(cost, torch.Tensor) or cost.dim() != 2 or cost.shape[0] != cost.shape[1]:
        raise ValueError(f'cost must be a square tensor [n,n], got {tuple(getattr(cost, "shape", ()))}')
    n = int(cost.shape[0])
    if n > MATCH_MAX_BOXES:
        raise ValueError(f'{n} boxes: matching takes at most {MATCH_MAX_BOXES}')
    n_views = _check_n_views(n_views, 0)
    dev = cost.device
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    person_index, n_persons, rows, starts = i32(n), i32(1), i32(n * n_views), i32(n + 1)
    if n == 0:
        n_persons.zero_()
        starts.zero_()
        return person_index, n_persons, rows, starts
    cost = cost.to(torch.float32).contiguous()
    check(_lib.load().metro_cluster_views(_p(cost), n, n_views, float(max_cost_mm), _p(person_index), _p(n_persons), _p(rows),
                                          _p(starts), _stream(dev)), 'metro_cluster_views')
    return person_index, n_persons, rows, starts


def person_steps(rows, starts, n_persons, box_step, step_times, n_views: int = 1):
    """The time step of every person cluster_views found, and the persons as the time-step CSR associate_tracks reads, one
    metro_person_steps launch (one workgroup): no host work between clustering and association.  rows, starts [n + 1] and
    n_persons [1]: cluster_views' CSR and count, device tensors, n <= 128 the upper bound of the persons; box_step [n_boxes]
    (ints or a tensor): the step of each box; step_times [S] seconds, ascending (host values or a tensor).
    -> (person_step int32 [n]: the smallest step among the boxes of the person's group, -1 for persons at or past the count
    and for empty groups (a person seen by one camera); person_times float64 [n]: step_times of that step, NaN where it is
    -1; step_rows int32 [n]: the persons with a step sorted by (step, person), -1 past their number; step_starts int32
    [S + 1], step_starts[S] the number of persons with a step), all on the device.  Row and step values out of range are
    skipped.  associate_tracks takes person_times, step_rows and step_starts as they are."""
    if not isinstance(starts, torch.Tensor) or not isinstance(rows, torch.Tensor) or not isinstance(n_persons, torch.Tensor):
        raise ValueError('rows, starts and n_persons must be the device tensors cluster_views returned')
    if starts.numel() < 1 or n_persons.numel() != 1:
        raise ValueError(f'starts must hold n + 1 offsets and n_persons one count, got {starts.numel()} and {n_persons.numel()}')
    n = int(starts.numel()) - 1
    if n > MATCH_MAX_BOXES:
        raise ValueError(f'{n} persons: matching takes at most {MATCH_MAX_BOXES}')
    n_views = _check_n_views(n_views, int(rows.numel()))
    dev = starts.device
    rows, starts, n_persons = _i32(rows, dev).reshape(-1), _i32(starts, dev).reshape(-1), _i32(n_persons, dev).reshape(-1)
    box_step = _i32(box_step, dev).reshape(-1)
    step_times, out = _person_step_outputs(n, step_times, dev)
    if n:
        check(_lib.load().metro_person_steps(_p(rows), rows.numel(), _p(starts), _p(n_persons), n, n_views, _p(box_step), box_step.numel(),
                                             _p(step_times), step_times.numel(), *(_p(t) for t in out), _stream(dev)), 'metro_person_steps')
    return out


def _person_step_outputs(n: int, step_times, dev):
    """step_times [S] as a float64 device tensor, and what person_steps* write over n persons: (person_step, person_times, step_rows,
    step_starts), step_starts zeroed where n = 0 leaves nothing to launch."""
    if not isinstance(step_times, torch.Tensor):
        step_times = torch.from_numpy(np.ascontiguousarray(np.asarray(step_times, np.float64).reshape(-1)))
    step_times = step_times.to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    out = (i32(n), torch.empty((n,), dtype=torch.float64, device=dev), i32(n), i32(step_times.numel() + 1))
    if n == 0:
        out[3].zero_()
    return step_times, out


def person_steps_labels(person_index, n_persons, box_step, step_times):
    """person_steps from the persons' labels alone, one metro_person_steps_labels launch (one workgroup): a person ONE camera
    sees gets a step too.  person_index [n] and n_persons [1]: cluster_views' labels and count, device tensors, n <= 128;
    box_step [n] (ints or a tensor) and step_times [S] as person_steps reads them.
    -> (person_step, person_times, step_rows, step_starts) as person_steps returns them -- for a person with several boxes the
    same values -- and single_box int32 [n]: the box of a person that has exactly one box, and a valid step; -1 for everyone
    else.  Labels and steps out of range are skipped.  (A function of its own: person_steps' parameter list is pinned.)"""
    if not isinstance(person_index, torch.Tensor) or not isinstance(n_persons, torch.Tensor):
        raise ValueError('person_index and n_persons must be the device tensors cluster_views returned')
    if person_index.dim() != 1 or n_persons.numel() != 1:
        raise ValueError(f'person_index must be [n] and n_persons hold one count, got {tuple(person_index.shape)} and {n_persons.numel()}')
    n = int(person_index.numel())
    if n > MATCH_MAX_BOXES:
        raise ValueError(f'{n} persons: matching takes at most {MATCH_MAX_BOXES}')
    dev = person_index.device
    person_index, n_persons = _i32(person_index, dev), _i32(n_persons, dev).reshape(-1)
    box_step = _i32(box_step, dev).reshape(-1)
    if box_step.numel() != n:
        raise ValueError(f'box_step must hold one value per box ({n}), got {box_step.numel()}')
    step_times, out = _person_step_outputs(n, step_times, dev)
    out += (torch.empty((n,), dtype=torch.int32, device=dev),)                      # single_box
    if n:
        check(_lib.load().metro_person_steps_labels(_p(person_index), _p(n_persons), n, _p(box_step), n, _p(step_times), step_times.numel(),
                                                    *(_p(t) for t in out), _stream(dev)), 'metro_person_steps_labels')
    return out


PERSON_RAY_DOUBLES = 8               # per (person, joint): o (3), d (3), sigma2, the number of views used


def person_rays(coords01: torch.Tensor, cov01: Optional[torch.Tensor], places: torch.Tensor, single_box: torch.Tensor,
                spec: ModelSpec, n_views: int = 1, weights: str = 'covariance') -> torch.Tensor:
    """The ray of every joint of the persons one camera sees, one metro_person_rays launch.  coords01 [m,J_head,3], cov01
    [m,J_head,6] (weights 'covariance') and `places` (m MetroPlacement records, uint8) as triangulate_joints reads them,
    m = n * n_views crop rows, box-major; single_box int32 [n] on the device (person_steps_labels): the one box of person p,
    -1 none.  -> rays float64 [n,Jout,8] on the device: the optical centre o (3) of the box's crops, the unit direction d (3) --
    the views' directions averaged with weights 1 ('uniform') or 1 / sigma2_v ('covariance'), the mirror joint for a flipped
    view --, sigma2 (the lateral variance of the ray in normalised image units, 1 / sum (1 / sigma2_v); 0 with 'uniform') and the
    number of views used.  All eight NaN where there is no ray: single_box -1, or no usable view."""
    triangulation_min_det(weights, 2.0)
    m, n_views, n = _checked_crop_rows(coords01, cov01, places, spec, n_views, weights)
    if not isinstance(single_box, torch.Tensor) or single_box.numel() != n:
        raise ValueError(f'single_box must be a device tensor of one value per person ({n})')
    dev = coords01.device
    rays = torch.empty((n, spec.skeleton.n_out, PERSON_RAY_DOUBLES), dtype=torch.float64, device=dev)
    if n == 0:
        return rays
    single_box = _i32(single_box, dev).reshape(-1)
    coords01, places = coords01.to(torch.float32).contiguous(), places.contiguous()
    cov01 = cov01.to(torch.float32).contiguous() if weights == 'covariance' else None
    cs = spec.to_c(1)
    mirror = _table(spec.skeleton.out_mirror, np.int32, dev)
    check(_lib.load().metro_person_rays(_p(coords01), _p(cov01), _p(places), m, C.byref(cs), _p(mirror), TRI_WEIGHTS[weights],
                                        _p(single_box), n, n_views, _p(rays), _stream(dev)), 'metro_person_rays')
    return rays


SMOOTH_MODES = {'filter': _lib.METRO_SMOOTH_FILTER, 'smooth': _lib.METRO_SMOOTH_RTS}
SMOOTH_MEASUREMENTS = {'isotropic': _lib.METRO_SMOOTH_ISOTROPIC, 'covariance': _lib.METRO_SMOOTH_COVARIANCE}
TRACK_STATE_DOUBLES = 28             # per (track, joint): x (6), the upper triangle of P (21), t_last


def _positive(name, v, zero_ok=False) -> float:
    ok = not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating)) and np.isfinite(v)
    if not ok or v < 0 or (v == 0 and not zero_ok):
        raise ValueError(f"{name} must be a finite number {'>= 0' if zero_ok else '> 0'}, got {v!r}")
    return float(v)


def smoothing_params(mode, measurement, accel_psd, sigma_floor_mm, cov_scale, initial_speed_mm_s, gate):
    """Checks the smoothing keywords of smooth_tracks / frames.track_poses_in_frames; -> metro_smooth_tracks' (mode,
    measurement, q, r_floor, cov_scale, v0, gate), gate None as 0."""
    if not isinstance(mode, str) or mode not in SMOOTH_MODES:
        raise ValueError(f"mode must be 'smooth' or 'filter', got {mode!r}")
    if not isinstance(measurement, str) or measurement not in SMOOTH_MEASUREMENTS:
        raise ValueError(f"measurement must be 'covariance' or 'isotropic', got {measurement!r}")
    return (SMOOTH_MODES[mode], SMOOTH_MEASUREMENTS[measurement], _positive('accel_psd', accel_psd),
            _positive('sigma_floor_mm', sigma_floor_mm), _positive('cov_scale', cov_scale, zero_ok=True),
            _positive('initial_speed_mm_s', initial_speed_mm_s), 0.0 if gate is None else _positive('gate', gate))


class Smoothing(NamedTuple):
    """The smoothing keywords of smooth_tracks and the follow calls, checked once, where the group is built (`checked`, which
    keeps the numbers as smoothing_params returns them: floats, gate None as 0)."""
    mode: str
    measurement: str
    accel_psd: float
    sigma_floor_mm: float
    cov_scale: float
    initial_speed_mm_s: float
    gate: float

    @classmethod
    def checked(cls, mode, measurement, *numbers) -> 'Smoothing':
        return cls(mode, measurement, *smoothing_params(mode, measurement, *numbers)[2:])

    def params(self):
        """metro_smooth_tracks' (mode, measurement, q, r_floor, cov_scale, v0, gate)."""
        return (SMOOTH_MODES[self.mode], SMOOTH_MEASUREMENTS[self.measurement], *self[2:])


def _checked_rows(poses, covariance, with_cov: bool, times, rows, starts, starts_name: str, groups: str):
    """What smooth_tracks and _associate_tracks check alike: poses [n,J,3], the covariance a 'covariance' measurement needs, one
    time per row and a CSR of at least one offset -> (n, J, times as a tensor, len(rows), len(starts))."""
    if not isinstance(poses, torch.Tensor) or poses.dim() != 3 or poses.shape[2] != 3 or not 1 <= poses.shape[1] <= _lib.METRO_MAX_JOINTS:
        raise ValueError(f'poses must be a tensor [n,J,3] with J <= {_lib.METRO_MAX_JOINTS}, got {tuple(getattr(poses, "shape", ()))}')
    n, nj = int(poses.shape[0]), int(poses.shape[1])
    if with_cov and (covariance is None or tuple(covariance.shape) not in ((n, nj, 3, 3), (n, nj, 9))):
        raise ValueError(f"measurement='covariance' needs covariance [{n},{nj},3,3], got "
                         f'{None if covariance is None else tuple(covariance.shape)}')
    if not isinstance(times, torch.Tensor):
        times = torch.from_numpy(np.ascontiguousarray(np.asarray(times, np.float64).reshape(-1)))
    if times.numel() != n:
        raise ValueError(f'times must hold one value per pose row ({n}), got {times.numel()}')
    n_rows = int(rows.numel() if isinstance(rows, torch.Tensor) else np.asarray(rows).size)
    n_starts = int(starts.numel() if isinstance(starts, torch.Tensor) else np.asarray(starts).size)
    if n_starts < 1:
        raise ValueError(f'{starts_name} must hold {groups} + 1 offsets ({groups} >= 0)')
    return n, nj, times, n_rows, n_starts


def smooth_tracks(poses: torch.Tensor, covariance: Optional[torch.Tensor], times, rows, starts, mode: str = 'smooth',
                  measurement: str = 'covariance', accel_psd: float = 4e6, sigma_floor_mm: float = 1.0, cov_scale: float = 1.0,
                  initial_speed_mm_s: float = 2000.0, gate: Optional[float] = None, state: Optional[torch.Tensor] = None):
    """Poses of tracked persons filtered over time, one metro_smooth_tracks launch (include/metro_hip.h has the model).
    poses [n,J,3] mm and (measurement 'covariance') covariance [n,J,3,3] or [n,J,9] mm^2 on the device, as
    locate_poses_in_frames(return_uncertainty=True) returns them; times [n] seconds (host values or a tensor); track t owns
    the rows rows[starts[t]:starts[t+1]] in time order (frames.track_groups; int arrays or tensors, starts [T+1]).
    -> (poses [n,J,3], velocity [n,J,3] mm/s, covariance [n,J,3,3] mm^2 of the position, used uint8 [n,J]).
    Per track and joint a constant-velocity Kalman filter reads each row's pose as a measurement with noise
    R = cov_scale * covariance + sigma_floor_mm^2 I ('isotropic': sigma_floor_mm^2 I); mode 'filter' returns the causal
    estimates, 'smooth' (default) the Rauch-Tung-Striebel smoothed ones.  A row whose pose is non-finite, or whose R is not
    positive definite, is bridged by the prediction (used 0), as is one whose innovation exceeds `gate` (a squared
    Mahalanobis distance, chi-square with 3 degrees of freedom; None: no gate); rows before a track's first usable
    measurement are NaN.  Rows in no group come back as given: their pose, NaN velocity, their R, used 0.
    The defaults are design choices, not measurements: accel_psd = 4e6 mm^2/s^3 is the white-noise acceleration density
    that roughly 2 m/s^2 sustained over a second amounts to; sigma_floor_mm = 1 keeps R positive definite without
    outweighing any real heat-map; initial_speed_mm_s = 2000 is the prior spread of the unknown first velocity.
    state: None, or a float64 [T,J,28] device tensor (frames.new_track_state) carried from call to call: a track whose slot
    holds a state continues from it, and every track with rows in this call gets the FILTER state of its last row written
    back in place (in both modes), so a stream cut into calls is filtered as one."""
    return _smooth_tracks(poses, covariance, times, rows, starts,
                          Smoothing.checked(mode, measurement, accel_psd, sigma_floor_mm, cov_scale, initial_speed_mm_s, gate), state)


def _smooth_tracks(poses, covariance, times, rows, starts, smoothing: Smoothing, state):
    """smooth_tracks on a checked Smoothing group."""
    params, with_cov = smoothing.params(), smoothing.measurement == 'covariance'
    n, nj, times, n_rows, n_starts = _checked_rows(poses, covariance, with_cov, times, rows, starts, 'starts', 'T')
    dev, n_tracks = poses.device, n_starts - 1
    if state is not None and (not isinstance(state, torch.Tensor) or state.dtype != torch.float64 or state.device != dev
                              or tuple(state.shape) != (n_tracks, nj, TRACK_STATE_DOUBLES) or not state.is_contiguous()):
        raise ValueError(f'state must be a contiguous float64 tensor [{n_tracks},{nj},{TRACK_STATE_DOUBLES}] on {dev} '
                         '(frames.new_track_state)')
    lib = _lib.load()
    times = times.to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
    rows, starts = _i32(rows, dev).reshape(-1), _i32(starts, dev).reshape(-1)
    poses = poses.to(torch.float32).contiguous()
    cov = covariance.to(torch.float32).reshape(n, nj, 9).contiguous() if with_cov else None
    # what the launch leaves alone: rows in no group keep their pose, a NaN velocity, their R and used = 0
    out = poses.clone()
    velocity = torch.full_like(poses, float('nan'))
    r = torch.eye(3, dtype=torch.float32, device=dev).mul(params[3] ** 2).expand(n, nj, 3, 3)
    if with_cov:
        upper = cov.view(n, nj, 3, 3).triu()
        r = r + params[4] * (upper + upper.triu(1).transpose(-1, -2))
    cov_out = r.reshape(n, nj, 9).contiguous()
    used = torch.zeros((n, nj), dtype=torch.uint8, device=dev)
    ws = torch.empty(lib.metro_smooth_tracks_workspace_bytes(n_rows, nj) if smoothing.mode == 'smooth' else 0, dtype=torch.uint8, device=dev)
    cs = _lib.MetroSpec(n_joints_out=nj)
    check(lib.metro_smooth_tracks(_p(poses), _p(cov), _p(times), n, _p(rows), n_rows, _p(starts), n_tracks, C.byref(cs), *params,
                                  _p(state), _p(ws), _p(out), _p(velocity), _p(cov_out), _p(used), _stream(dev)),
          'metro_smooth_tracks')
    return out, velocity, cov_out.view(n, nj, 3, 3), used


ASSOC_MAX = _lib.METRO_ASSOC_MAX       # boxes per time step, and track slots, of associate_tracks


class AssociatedTracks(NamedTuple):
    """What associate_tracks returns, all on the device."""
    track_index: torch.Tensor            # int32 [n]: the slot of every box, -1 untracked
    track_id: torch.Tensor               # int32 [n]: the persistent id of its track, -1 untracked
    cost: torch.Tensor                   # float32 [n] mm: the accepted cost of a box that continues a track, NaN for births / untracked
    rows: torch.Tensor                   # int32 [n] and
    starts: torch.Tensor                 # int32 [T + 1]: the CSR per slot in time order that smooth_tracks reads; rows past starts[T] are -1
    n_new: torch.Tensor                  # int32 [1]: tracks born in this call
    n_dropped: torch.Tensor              # int32 [1]: boxes left untracked (no free slot, or no finite joint)
    working_state: torch.Tensor          # float64 [T, J, 28]: the state as the launch advanced it (what smooth_tracks will leave in `state`)


def association_params(max_cost_mm, clip_mm, min_joints, max_age_s):
    """Checks the association keywords of associate_tracks / frames.follow_poses_in_frames."""
    matching_params(clip_mm, min_joints, max_cost_mm)
    ok = not isinstance(max_age_s, (bool, np.bool_)) and isinstance(max_age_s, (int, float, np.integer, np.floating))
    if not ok or np.isnan(max_age_s) or max_age_s < 0:
        raise ValueError(f'max_age_s must be a number >= 0 (seconds), got {max_age_s!r}')


ASSIGNMENTS = ('greedy', 'optimal')


def assignment_rule(assignment):
    """Checks the `assignment` keyword of associate_tracks, frames.follow_world_poses_in_frames and frames.Follower."""
    if not isinstance(assignment, str) or assignment not in ASSIGNMENTS:
        raise ValueError(f"assignment must be 'greedy' or 'optimal', got {assignment!r}")


class Association(NamedTuple):
    """The association keywords of associate_tracks* and the follow calls with the assignment rule, checked once, where the
    group is built (`checked`: the ray depth sigma, then the rule, then the rest).  ray_depth_sigma_mm is kept for a chain with
    ray rows (`rays`: associate_tracks_rays, single_view='rays') and None otherwise; given, it is checked either way."""
    max_cost_mm: float
    clip_mm: float
    min_joints: Optional[int]
    max_age_s: float
    assignment: str
    ray_depth_sigma_mm: Optional[float] = None

    @classmethod
    def checked(cls, max_cost_mm, clip_mm, min_joints, max_age_s, assignment, ray_depth_sigma_mm=None, rays=False) -> 'Association':
        if rays or ray_depth_sigma_mm is not None:
            ray_depth_sigma_mm = ray_depth_sigma(ray_depth_sigma_mm)
        assignment_rule(assignment)
        association_params(max_cost_mm, clip_mm, min_joints, max_age_s)
        return cls(max_cost_mm, clip_mm, min_joints, max_age_s, assignment, ray_depth_sigma_mm if rays else None)


def associate_tracks(poses: torch.Tensor, covariance: Optional[torch.Tensor], times, step_rows, step_starts, state: torch.Tensor,
                     ids: torch.Tensor, next_id: torch.Tensor, max_cost_mm: float = 300.0, clip_mm: float = 600.0,
                     min_joints: Optional[int] = None, max_age_s: float = 1.0, measurement: str = 'covariance',
                     accel_psd: float = 4e6, sigma_floor_mm: float = 1.0, cov_scale: float = 1.0,
                     initial_speed_mm_s: float = 2000.0, gate: Optional[float] = None,
                     assignment: str = 'greedy') -> AssociatedTracks:
    """Which box of a video continues which track, one metro_associate_tracks launch (one workgroup, the cost matrix in LDS;
    include/metro_hip.h has the model).  poses [n,J,3] mm ABSOLUTE, covariance and times as smooth_tracks reads them;
    step s owns the boxes step_rows[step_starts[s]:step_starts[s+1]], the steps in ascending time, all boxes of one
    timestamp in one step (frames.time_steps; at most 128 boxes per step).  The track table (frames.new_track_table) is
    state float64 [T,J,28] (smooth_tracks' carried state), ids int32 [T] (-1: free) and next_id int32 [1], T <= 128, all on
    the device of `poses`; ids and next_id are updated in place, and of `state` only the t_last of slots retired at the
    start (last seen more than max_age_s before the call's first box).
    Per step: the cost of a slot continuing in a box is the RMS over the joints of the distance between the box's joint and
    the slot's constant-velocity prediction, each capped at clip_mm (+inf from fewer than min_joints joints -- None:
    (J + 1) // 2 -- or for a slot last seen more than max_age_s ago); boxes and slots are paired greedily, smallest cost
    first, while it is below max_cost_mm; the remaining boxes start new tracks in the lowest free slots; every slot that got
    a box advances a working copy of the state by smooth_tracks' filter step, with the same measurement, accel_psd,
    sigma_floor_mm, cov_scale, initial_speed_mm_s and gate.
    assignment 'greedy' (the default): that pairing, which is not an optimal assignment -- with tracks A at x = 0 and B at
    x = 230 mm and boxes at -120 and +100 it takes A-(+100) at 100 mm, after which B has no box within max_cost_mm: A continues
    in B's box, A's own box is born under a new id and B is bridged.  assignment 'optimal' (one
    metro_associate_tracks_optimal launch, the same workgroup and cost matrix): with g = max_cost_mm a pair is admissible if
    its cost c < g, and the pairing is the one-to-one set of admissible pairs that minimises the sum of (c - g), i.e.
    maximises the total gain sum (g - c) -- the linear assignment problem on min(c, g) in which a pair at g means
    "unmatched", solved exactly by shortest augmenting paths in fp64; above it keeps both ids, at 120 + 130 mm.  This is
    not a maximum-cardinality matching: one pair at 10 mm beats two at 299 mm each.  Costs, births, n_dropped, the filter
    step and the CSR are the same code under both rules.
    max_cost_mm = 300, clip_mm = 600, max_age_s = 1 and the min_joints default are design choices, not measurements: 300 mm
    is below the distance between two persons side by side and above what a person's joints move against a constant-velocity
    prediction within a few frames; 600 mm keeps one wild joint from deciding a pair; one second bridges a short occlusion
    without handing a long-gone track's slot history to a newcomer; half the joints keeps a cost from resting on a few.
    -> AssociatedTracks; its rows / starts and `state` go to smooth_tracks unchanged.  No boxes or no steps: no launch."""
    return _associate_tracks(poses, covariance, times, step_rows, step_starts, state, ids, next_id,
                             Association.checked(max_cost_mm, clip_mm, min_joints, max_age_s, assignment),
                             Smoothing.checked('filter', measurement, accel_psd, sigma_floor_mm, cov_scale, initial_speed_mm_s, gate))


class RayAssociatedTracks(NamedTuple):
    """What associate_tracks_rays returns, all on the device: AssociatedTracks' fields, then the additions."""
    track_index: torch.Tensor
    track_id: torch.Tensor
    cost: torch.Tensor
    rows: torch.Tensor
    starts: torch.Tensor
    n_new: torch.Tensor
    n_dropped: torch.Tensor              # int32 [1]: POINT rows left untracked; an untracked ray row counts in n_unplaced
    working_state: torch.Tensor
    poses: torch.Tensor                  # float32 [n, J, 3]: a copy of the given poses with the placed joints of the ray rows written
    covariance: torch.Tensor             # float32 [n, J, 9]: likewise, their R; both go to smooth_tracks with rows / starts
    ray_depth: torch.Tensor              # float32 [n, J] mm: the depth tau along the ray at which a joint was placed, NaN elsewhere
    n_unplaced: torch.Tensor             # int32 [1]: ray rows no track continued in (a ray row is never born)


def ray_depth_sigma(ray_depth_sigma_mm) -> float:
    """Checks `ray_depth_sigma_mm` of associate_tracks_rays and frames.follow_rig_poses_in_frames."""
    if not _is_number(ray_depth_sigma_mm) or not np.isfinite(ray_depth_sigma_mm) or not ray_depth_sigma_mm > 0:
        raise ValueError(f'ray_depth_sigma_mm must be a finite number > 0 (mm), got {ray_depth_sigma_mm!r}')
    return float(ray_depth_sigma_mm)


def associate_tracks_rays(poses: torch.Tensor, covariance: torch.Tensor, times, step_rows, step_starts, state: torch.Tensor,
                          ids: torch.Tensor, next_id: torch.Tensor, single_box: torch.Tensor, rays: torch.Tensor,
                          max_cost_mm: float = 300.0, clip_mm: float = 600.0, min_joints: Optional[int] = None,
                          max_age_s: float = 1.0, accel_psd: float = 4e6, sigma_floor_mm: float = 1.0, cov_scale: float = 1.0,
                          initial_speed_mm_s: float = 2000.0, gate: Optional[float] = None, assignment: str = 'greedy',
                          ray_depth_sigma_mm: float = 1000.0) -> RayAssociatedTracks:
    """associate_tracks with RAY rows among the boxes, one metro_associate_tracks_rays launch (include/metro_hip.h has the
    model): row b with single_box[b] >= 0 (person_steps_labels) is a person one camera sees, with no pose but one ray per
    joint, rays [n,J,8] (person_rays).  Every other row, the table and every other keyword are associate_tracks'; the
    measurement is 'covariance' (an isotropic R would ignore the ray's shape and pin the depth along it).
    A ray row costs a slot the RMS over the joints of the distance of the slot's predicted joint from the ray (clip_mm behind
    the camera) -- blind along the ray --, competes with the point rows in the one assignment (either rule), is never born (no
    depth to start from; unassigned it counts in n_unplaced), and once assigned each of its joints is PLACED: the pose becomes
    the foot of the perpendicular from the predicted joint onto the ray, at depth tau, and its covariance
    R = sigma2 tau^2 (I - d d^T) + ray_depth_sigma_mm^2 d d^T, tight across the ray and wide along it (the linearised form of
    a bearing measurement), which the unchanged filter step then reads.  The launch works on copies of `poses` and
    `covariance` and returns them: smooth_tracks on them with rows / starts leaves the working state in `state`, bit for bit.
    ray_depth_sigma_mm = 1000 is a design choice, not a measurement: the placed point has no innovation along the ray, so the
    along-ray variance only has to be large against the predicted P there (tens of mm) for the update to leave the depth to
    the motion model -- at 1 m the gain along the ray is below 1e-2 -- and small enough that the fp32 rounding of R's entries
    (one ulp at 1e6 mm^2 is 0.06 mm^2) stays far below sigma_floor_mm^2 and the lateral variance.
    -> RayAssociatedTracks."""
    depth_sigma = ray_depth_sigma(ray_depth_sigma_mm)
    if not isinstance(poses, torch.Tensor) or poses.dim() != 3:
        raise ValueError(f'poses must be a tensor [n,J,3], got {tuple(getattr(poses, "shape", ()))}')
    n, nj = int(poses.shape[0]), int(poses.shape[1])
    if not isinstance(single_box, torch.Tensor) or single_box.numel() != n:
        raise ValueError(f'single_box must be a device tensor of one value per pose row ({n})')
    if not isinstance(rays, torch.Tensor) or rays.dtype != torch.float64 or tuple(rays.shape) != (n, nj, PERSON_RAY_DOUBLES):
        raise ValueError(f'rays must be a float64 tensor [{n},{nj},{PERSON_RAY_DOUBLES}] (person_rays), got '
                         f'{tuple(getattr(rays, "shape", ()))}')
    return _associate_tracks(poses, covariance, times, step_rows, step_starts, state, ids, next_id,
                             Association.checked(max_cost_mm, clip_mm, min_joints, max_age_s, assignment)._replace(
                                 ray_depth_sigma_mm=depth_sigma),
                             Smoothing.checked('filter', 'covariance', accel_psd, sigma_floor_mm, cov_scale, initial_speed_mm_s, gate),
                             (single_box, rays))


def _associate_tracks(poses, covariance, times, step_rows, step_starts, state, ids, next_id, association: Association,
                      smoothing: Smoothing, rays=None):
    """associate_tracks (rays None) and associate_tracks_rays (rays = (single_box, rays), the depth sigma the association's: the
    launch writes copies of poses and covariance) on checked groups; the filter step reads `smoothing` without its mode."""
    max_cost_mm, clip_mm, min_joints, max_age_s, assignment, depth_sigma = association
    params, with_cov = smoothing.params(), smoothing.measurement == 'covariance'
    n, nj, times, n_step_rows, n_starts = _checked_rows(poses, covariance, with_cov, times, step_rows, step_starts, 'step_starts', 'S')
    if min_joints is None:
        min_joints = (nj + 1) // 2
    if min_joints > nj:
        raise ValueError(f'min_joints must be at most the {nj} joints, got {min_joints!r}')
    dev = poses.device
    if not isinstance(step_starts, torch.Tensor):
        sizes = np.diff(np.asarray(step_starts, np.int64).reshape(-1))
        if len(sizes) and sizes.max() > ASSOC_MAX:
            raise ValueError(f'{int(sizes.max())} boxes in one time step: association takes at most {ASSOC_MAX}')
    if (not isinstance(state, torch.Tensor) or state.dtype != torch.float64 or state.dim() != 3 or state.device != dev
            or tuple(state.shape[1:]) != (nj, TRACK_STATE_DOUBLES) or not state.is_contiguous() or not 1 <= state.shape[0] <= ASSOC_MAX):
        raise ValueError(f'state must be a contiguous float64 tensor [T,{nj},{TRACK_STATE_DOUBLES}] on {dev} with 1 <= T <= {ASSOC_MAX} '
                         '(frames.new_track_table)')
    n_tracks = int(state.shape[0])
    for name, t, size in (('ids', ids, n_tracks), ('next_id', next_id, 1)):
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.device != dev or t.numel() != size or not t.is_contiguous()):
            raise ValueError(f'{name} must be a contiguous int32 tensor of {size} on {dev} (frames.new_track_table)')
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    track_index, track_id, rows, starts, n_new, n_dropped = i32(n), i32(n), i32(n), i32(n_tracks + 1), i32(1), i32(1)
    cost = torch.empty((n,), dtype=torch.float32, device=dev)
    if n == 0 or n_step_rows == 0 or n_starts == 1:        # nothing to decide: no launch
        track_index.fill_(-1), track_id.fill_(-1), rows.fill_(-1), cost.fill_(float('nan'))
        starts.zero_(), n_new.zero_(), n_dropped.zero_()
        found = AssociatedTracks(track_index, track_id, cost, rows, starts, n_new, n_dropped, state.clone())
        if rays is None:
            return found
        return RayAssociatedTracks(*found, poses.to(torch.float32).clone(), covariance.to(torch.float32).reshape(n, nj, 9).clone(),
                                   torch.full((n, nj), float('nan'), dtype=torch.float32, device=dev), i32(1).zero_())
    lib = _lib.load()
    times = times.to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
    step_rows, step_starts = _i32(step_rows, dev).reshape(-1), _i32(step_starts, dev).reshape(-1)
    ws = torch.empty(lib.metro_associate_tracks_workspace_bytes(n_tracks, nj), dtype=torch.uint8, device=dev)
    cs = _lib.MetroSpec(n_joints_out=nj)
    found = AssociatedTracks(track_index, track_id, cost, rows, starts, n_new, n_dropped,
                             ws.view(torch.float64).view(n_tracks, nj, TRACK_STATE_DOUBLES))
    shared = (_p(times), n, _p(step_rows), n_step_rows, _p(step_starts), n_starts - 1, C.byref(cs), *params[1:], float(max_cost_mm),
              float(clip_mm), int(min_joints), float(max_age_s), _p(state), n_tracks, _p(ids), _p(next_id), _p(ws),
              *(_p(t) for t in found[:7]))                  # every entry's arguments between (poses, cov) and its own tail
    if rays is not None:
        poses = poses.to(torch.float32).clone(memory_format=torch.contiguous_format)
        cov = covariance.to(torch.float32).reshape(n, nj, 9).clone(memory_format=torch.contiguous_format)
        single_box, ray = _i32(rays[0], dev).reshape(-1), rays[1].contiguous()
        ray_depth, n_unplaced = torch.empty((n, nj), dtype=torch.float32, device=dev), i32(1)
        check(lib.metro_associate_tracks_rays(_p(poses), _p(cov), *shared, int(assignment == 'optimal'), _p(single_box), _p(ray),
                                              depth_sigma, _p(ray_depth), _p(n_unplaced), _stream(dev)), 'metro_associate_tracks_rays')
        return RayAssociatedTracks(*found, poses, cov, ray_depth, n_unplaced)
    poses = poses.to(torch.float32).contiguous()
    cov = covariance.to(torch.float32).reshape(n, nj, 9).contiguous() if with_cov else None
    entry = 'metro_associate_tracks_optimal' if assignment == 'optimal' else 'metro_associate_tracks'
    check(getattr(lib, entry)(_p(poses), _p(cov), *shared, _stream(dev)), entry)
    return found


BONE_STAT_DOUBLES = 4                # per (track slot, edge): S0 = sum 1/v, S1 = sum l/v, count, rejected


class BoneLengths(NamedTuple):
    """What track_bone_lengths returns, all on the device."""
    lengths: torch.Tensor                # float64 [T, E] mm: the learned length, the fallback (NaN without one) where it is not known
    sigma: torch.Tensor                  # float64 [T, E] mm: the standard error the weights imply, NaN where it is not known
    known: torch.Tensor                  # uint8 [T, E]: 1 where at least min_count rows (with the mirror bone's) were accepted


def bone_length_params(min_count=8, gate=9.0, sigma_floor_mm=1.0, cov_scale=1.0, min_length_mm=1.0, debias=True, symmetric=True):
    """Checks the estimator keywords of track_bone_lengths / frames.Follower(learn_bones=True); -> metro_track_bone_lengths'
    (min_count, gate, r_floor, cov_scale, min_length_mm, debias, symmetric), gate None as 0."""
    if isinstance(min_count, (bool, np.bool_)) or not isinstance(min_count, (int, np.integer)) or min_count < 1:
        raise ValueError(f'min_count must be an integer >= 1, got {min_count!r}')
    for name, flag in (('debias', debias), ('symmetric', symmetric)):
        if not isinstance(flag, (bool, np.bool_)):
            raise ValueError(f'{name} must be True or False, got {flag!r}')
    return (int(min_count), 0.0 if gate is None else _positive('gate', gate, zero_ok=True), _positive('sigma_floor_mm', sigma_floor_mm),
            _positive('cov_scale', cov_scale, zero_ok=True), _positive('min_length_mm', min_length_mm, zero_ok=True), int(debias),
            int(symmetric))


def bone_fallback(fallback, n_edges: Optional[int], required: bool = False) -> Optional[np.ndarray]:
    """Checks a `fallback` table: host float64 [E] mm, finite and positive (None unless `required`; n_edges None: any E >= 1)."""
    if fallback is None and not required:
        return None
    if fallback is None:
        raise ValueError('fallback is required: [E] bone lengths in mm for unknown tracks and edges')
    if isinstance(fallback, torch.Tensor):
        fallback = fallback.detach().cpu().numpy()
    f = np.asarray(fallback, np.float64)
    if f.ndim != 1 or len(f) < 1 or (n_edges is not None and len(f) != n_edges) or not (np.isfinite(f).all() and (f > 0).all()):
        raise ValueError(f"fallback must be [{'E' if n_edges is None else n_edges}] finite and positive bone lengths in mm, got "
                         f'shape {f.shape}')
    return np.ascontiguousarray(f)


def track_bone_lengths(poses: Optional[torch.Tensor], covariance: Optional[torch.Tensor], rows, starts, ids: torch.Tensor,
                       stats: torch.Tensor, bone_ids: torch.Tensor, edges, edge_mirror, fallback=None, min_count: int = 8,
                       gate: Optional[float] = 9.0, sigma_floor_mm: float = 1.0, cov_scale: float = 1.0, min_length_mm: float = 1.0,
                       debias: bool = True, symmetric: bool = True) -> BoneLengths:
    """The bone lengths of followed persons, learned per track slot: one metro_track_bone_lengths launch on the current stream,
    no synchronisation (include/metro_hip.h has the model and the reasoning).  poses [n,J,3] mm ABSOLUTE and covariance
    [n,J,3,3] or [n,J,9] mm^2 (None: isotropic) on the device -- the triangulation's own world poses and covariance, NaN where
    a joint could not be placed; rows / starts the CSR per slot associate_tracks* returned; ids int32 [T] the track table's ids
    after that association.  edges [E,2] in output joint indices (Skeleton.edges), edge_mirror [E] (Skeleton.edge_mirror()).
    The bone table (frames.new_bone_table), updated in place: stats float64 [T,E,4] = (S0, S1, count, rejected) and bone_ids
    int32 [T]: a slot whose id differs from bone_ids forgets first.  Per slot, edge and listed row the length l of the bone,
    corrected for the first-order bias of a noisy length (debias) to l^ = l - (tr C - u^T C u) / (2 l) with
    C = cov_scale (C_a + C_b), enters a mean weighted by 1 / v, v = tr C / 3 + sigma_floor_mm^2, unless it lies further than
    gate (a squared distance in units of v + 1/S0; None or 0: no gate) from the mean of at least min_count rows, which counts
    it in `rejected`.  Read-out: with `symmetric` a bone is pooled with its mirror bone; with at least min_count rows
    length = S1 / S0 and sigma = sqrt(1 / S0), known 1; else fallback [E] (NaN without one), known 0.
    poses None (or no rows): reset and read-out only.  min_count = 8, gate = 9 (3 sigma, one degree of freedom),
    min_length_mm = 1, sigma_floor_mm = 1 and cov_scale = 1 are design choices, not measurements.  -> BoneLengths."""
    params = bone_length_params(min_count, gate, sigma_floor_mm, cov_scale, min_length_mm, debias, symmetric)
    if (not isinstance(stats, torch.Tensor) or not stats.is_cuda or stats.dtype != torch.float64 or stats.dim() != 3
            or stats.shape[2] != BONE_STAT_DOUBLES or not 1 <= stats.shape[0] <= ASSOC_MAX or not 1 <= stats.shape[1] <= _lib.METRO_MAX_JOINTS or not stats.is_contiguous()):
        raise ValueError(f'stats must be a contiguous float64 CUDA tensor [T,E,{BONE_STAT_DOUBLES}] with 1 <= T <= {ASSOC_MAX} and '
                         f'1 <= E <= {_lib.METRO_MAX_JOINTS} (frames.new_bone_table)')
    dev, n_tracks, n_edges = stats.device, int(stats.shape[0]), int(stats.shape[1])
    for name, t in (('ids', ids), ('bone_ids', bone_ids)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.device != dev or t.numel() != n_tracks or not t.is_contiguous():
            raise ValueError(f'{name} must be a contiguous int32 tensor of {n_tracks} on {dev}')
    fallback = bone_fallback(fallback, n_edges)
    e = edges.detach().cpu().numpy() if isinstance(edges, torch.Tensor) else np.asarray(edges)
    em = edge_mirror.detach().cpu().numpy() if isinstance(edge_mirror, torch.Tensor) else np.asarray(edge_mirror)
    if e.shape != (n_edges, 2) or em.shape != (n_edges,):
        raise ValueError(f'edges must be [{n_edges},2] and edge_mirror [{n_edges}], got {e.shape} and {em.shape}')
    if poses is None:
        n = nj = n_rows = 0
    else:
        if not isinstance(poses, torch.Tensor) or poses.dim() != 3 or poses.shape[2] != 3 or not 1 <= poses.shape[1] <= _lib.METRO_MAX_JOINTS:
            raise ValueError(f'poses must be a tensor [n,J,3] with J <= {_lib.METRO_MAX_JOINTS}, got {tuple(getattr(poses, "shape", ()))}')
        n, nj = int(poses.shape[0]), int(poses.shape[1])
        if poses.device != dev:
            raise ValueError(f'poses are on {poses.device}, the bone table on {dev}')
        if covariance is not None and tuple(covariance.shape) not in ((n, nj, 3, 3), (n, nj, 9)):
            raise ValueError(f'covariance must be [{n},{nj},3,3] or None, got {tuple(covariance.shape)}')
        n_rows = int(rows.numel() if isinstance(rows, torch.Tensor) else np.asarray(rows).size)
        n_starts = int(starts.numel() if isinstance(starts, torch.Tensor) else np.asarray(starts).size)
        if n_starts != n_tracks + 1:
            raise ValueError(f'starts must hold T + 1 = {n_tracks + 1} offsets, got {n_starts}')
    from metro_pose3d_amd.frame_formats import _upload
    lib = _lib.load()
    e, em = np.ascontiguousarray(e, np.int32), np.ascontiguousarray(em, np.int32)
    # a skeleton's two small tables: uploaded once per device, complete before any stream reads them (_table) -- a non-blocking
    # upload cached here was ordered on the stream of the first call only, and a later call on another stream could read it early
    d_edges, d_mirror = _table(e.reshape(-1), np.int32, dev), _table(em, np.int32, dev)
    d_fallback = _upload(fallback, dev) if fallback is not None else None
    d_poses = d_cov = d_rows = d_starts = None
    if n > 0 and n_rows > 0:
        d_poses = poses.to(torch.float32).contiguous()
        d_cov = covariance.to(torch.float32).reshape(n, nj, 9).contiguous() if covariance is not None else None
        d_rows, d_starts = _i32(rows, dev).reshape(-1), _i32(starts, dev).reshape(-1)
    else:
        n = n_rows = 0
    lengths = torch.empty((n_tracks, n_edges), dtype=torch.float64, device=dev)
    sigma = torch.empty((n_tracks, n_edges), dtype=torch.float64, device=dev)
    known = torch.empty((n_tracks, n_edges), dtype=torch.uint8, device=dev)
    check(lib.metro_track_bone_lengths(_p(d_poses), _p(d_cov), n, _p(d_rows), n_rows, _p(d_starts), n_tracks, _p(ids), max(nj, 1),
                                       _p(d_edges), _p(d_mirror), n_edges, _p(d_fallback), *params, _p(stats), _p(bone_ids),
                                       _p(lengths), _p(sigma), _p(known), _stream(dev)), 'metro_track_bone_lengths')
    return BoneLengths(lengths, sigma, known)


PREDICT_MAX_DETECTIONS = _lib.METRO_PREDICT_MAX_DETECTIONS
FRAME_CAMERA_BYTES = C.sizeof(_lib.MetroFrameCamera)


class PredictedBoxRows(NamedTuple):
    """What predict_boxes returns, all on the device and unsliced: the first counts[0] rows hold the boxes."""
    boxes: torch.Tensor                  # float64 [F T + m, 4] (x, y, w, h)
    frame_index: torch.Tensor            # int32 [F T + m]
    track_index: torch.Tensor            # int32 [F T + m]: the slot of a predicted box, -1 for a detection
    track_id: torch.Tensor               # int32 [F T + m]: its id, -1 for a detection
    detection: torch.Tensor              # int32 [F T + m]: the index of a detection, -1 for a predicted box
    n_joints: torch.Tensor               # int32 [F T + m]: the visible joints of a predicted box, -1 for a detection
    dense_boxes: torch.Tensor            # float64 [F, T, 4]: the box of every (frame, slot), NaN where there is none
    dense_joints: torch.Tensor           # int32 [F, T]: its visible joints, -1: the slot is free or older than max_age_s
    counts: torch.Tensor                 # int32 [5]: rows, predicted rows, suppressed, bad detections, bad frame indices


def _finite(name, v, low, low_ok, high=None) -> float:
    ok = not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating)) and np.isfinite(v)
    if not ok or v < low or (v == low and not low_ok) or (high is not None and v > high):
        rng = f"{'>=' if low_ok else '>'} {low:g}" + ('' if high is None else f' and <= {high:g}')
        raise ValueError(f'{name} must be a finite number {rng}, got {v!r}')
    return float(v)


def prediction_params(expand, n_sigma, max_sigma_mm, min_joints, max_age_s, near_mm, min_side_px, iou_max, accel_psd):
    """Checks the prediction keywords of predict_boxes / frames.predict_boxes_in_frames; -> metro_predict_boxes' (q, max_age_s,
    expand, n_sigma, max_sigma_mm, near_mm, min_side_px) as floats, then iou_max.  min_joints: None or an integer >= 1."""
    if min_joints is not None and (isinstance(min_joints, (bool, np.bool_)) or not isinstance(min_joints, (int, np.integer))
                                   or min_joints < 1):
        raise ValueError(f'min_joints must be None or an integer >= 1, got {min_joints!r}')
    return (_finite('accel_psd', accel_psd, 0, False), _finite('max_age_s', max_age_s, 0, True), _finite('expand', expand, 1, True),
            _finite('n_sigma', n_sigma, 0, True), _finite('max_sigma_mm', max_sigma_mm, 0, True), _finite('near_mm', near_mm, 0, False),
            _finite('min_side_px', min_side_px, 0, True)), _finite('iou_max', iou_max, 0, False, 1)


TRACK_PRIOR_DEPTH = {'none': _lib.METRO_TRACK_PRIOR_DEPTH_NONE, 'root': _lib.METRO_TRACK_PRIOR_DEPTH_ROOT}
REASONS = ('prior given', 'no slot', 'no state', 'too old', 'behind or too near the camera', 'covariance not invertible',
           'non-finite input')                     # the reason words metro_plan_bind_track_prior writes, by value


def track_prior_params(coords='camera', depth='none', accel_psd=4e6, max_age_s=1.0, near_mm=100.0, sigma_floor_mm=30.0,
                       cov_scale=1.0) -> '_lib.MetroTrackPrior':
    """Checks the keywords of Engine.forward_track_posterior / frames.locate_tracked_poses_in_frames; -> the MetroTrackPrior
    record metro_plan_bind_track_prior copies.  coords: 'camera' or 'world', the frame of the track table ('crop' is refused: a
    crop's own camera differs from box to box, no table lives in it); depth: 'none' (no knowledge along z) or 'root' (z
    relative to the root, anchored at the root's plain coords01 z of the same forward); accel_psd > 0 and max_age_s >= 0 are the
    follow_* calls' own and should be theirs; near_mm > 0; sigma_floor_mm >= 0; cov_scale >= 0, and not both zero.
    The defaults sigma_floor_mm = 30, cov_scale = 1, near_mm = 100 and depth = 'none' are design choices, not measurements: a
    filter that has seen a joint a hundred times reports millimetres, less than a heat-map voxel and less than what a constant-
    velocity model misses of a limb that turns, and 30 mm (about one voxel of a 2.2 m box at S = 64) keeps such a prior from
    overruling the image; the predicted covariance is taken at face value; nothing nearer than 100 mm is a person in front of
    a lens (predict_boxes' rule); and z stays out of the prior unless asked for, because its anchor is the plain root mean."""
    if coords not in ('camera', 'world'):
        raise ValueError(f"coords must be 'camera' or 'world' (the frame of the track table; no table lives in a crop's), got {coords!r}")
    if depth not in TRACK_PRIOR_DEPTH:
        raise ValueError(f"depth must be 'none' or 'root', got {depth!r}")
    p = _lib.MetroTrackPrior()
    p.coords, p.depth = _COORDS[coords], TRACK_PRIOR_DEPTH[depth]
    p.accel_psd = _finite('accel_psd', accel_psd, 0, False)
    p.max_age_s = _finite('max_age_s', max_age_s, 0, True)
    p.near_mm = _finite('near_mm', near_mm, 0, False)
    p.sigma_floor_mm = _finite('sigma_floor_mm', sigma_floor_mm, 0, True)
    p.cov_scale = _finite('cov_scale', cov_scale, 0, True)
    if p.sigma_floor_mm == 0.0 and p.cov_scale == 0.0:
        raise ValueError('sigma_floor_mm and cov_scale are both 0: every prior would have a singular covariance')
    return p


FUSION_MAX_GRID = 16


class Fusion(NamedTuple):
    """The view-fusion keywords of Engine.forward_view_fusion / frames.fuse_poses_in_frames, checked (fusion_params)."""
    grid: int
    extent_mm: float
    floor: float
    near_mm: float

    def record(self, weights: str, min_angle_deg: float, n_views: int = 1) -> '_lib.MetroViewFusion':
        """The MetroViewFusion record metro_plan_bind_view_fusion copies, with the keywords of the internal triangulation and
        the rows per camera (test-time views: a row counts 1 / n_views)."""
        if isinstance(n_views, (bool, np.bool_)) or not isinstance(n_views, (int, np.integer)) or n_views < 1:
            raise ValueError(f'n_views must be an integer >= 1, got {n_views!r}')
        p = _lib.MetroViewFusion()
        p.min_det = triangulation_min_det(weights, min_angle_deg)          # checks both
        p.grid, p.n_views, p.weights = int(self.grid), int(n_views), TRI_WEIGHTS[weights]
        p.extent_mm, p.floor, p.near_mm = float(self.extent_mm), float(self.floor), float(self.near_mm)
        return p


def fusion_params(grid=16, extent_mm=1200.0, floor=1e-6, near_mm=100.0) -> Fusion:
    """Checks the keywords of Engine.forward_view_fusion / frames.fuse_poses_in_frames; -> Fusion.  grid: the points per axis
    of the cube of world points, an integer in [2, 16] (16^3 fp64 energies are the 32 KB of LDS the kernel keeps them in);
    extent_mm > 0: the cube's side, around the joint's triangulated point (or the centre the caller gives); floor in (0, 1): the
    least probability a camera gives a point -- what a point outside its map, behind it or on an empty cell counts, so that
    one camera that misses a joint cannot veto it; near_mm >= 0: a point nearer than this to a camera's plane takes the floor
    there.
    The defaults grid = 16, extent_mm = 1200, floor = 1e-6 and near_mm = 100 are design choices, not measurements: a 1.2 m cube
    in steps of 80 mm holds a wrong peak a few heat-map cells away at a person's distance (the `edge` output says when it did
    not); 1e-6 is far below a cell of any peaked 64 x 64 map and far above fp32's underflow; nothing nearer than 100 mm is a
    person in front of a lens (predict_boxes' rule).  One level only: a second, smaller grid around the first one's mode cut
    the distribution and biased its mean."""
    if isinstance(grid, (bool, np.bool_)) or not isinstance(grid, (int, np.integer)) or not 2 <= grid <= FUSION_MAX_GRID:
        raise ValueError(f'grid must be an integer in [2, {FUSION_MAX_GRID}], got {grid!r}')
    floor = _finite('floor', floor, 0, False, 1)
    if floor >= 1.0:
        raise ValueError(f'floor must lie in (0, 1), got {floor!r}')
    return Fusion(int(grid), _finite('extent_mm', extent_mm, 0, False), floor, _finite('near_mm', near_mm, 0, True))


SKELETON_MAX_EDGES = 63


def skeleton_mode_params(scale_mm, sigma_mm=20.0, sigma_rel=0.0, cov_scale=1.0, min_length_mm=1.0) -> '_lib.MetroSkeletonModes':
    """Checks the keywords of Engine.forward_skeleton_modes / estimate_pose_skeleton; -> the MetroSkeletonModes record
    metro_plan_bind_skeleton_modes copies.  scale_mm: three finite numbers > 0, mm per coords01 unit (the linear part of
    heatmap_to_metric); sigma_mm > 0: the sd of a bone's length; sigma_rel >= 0: the part of it that grows with the length
    (sd^2 = sigma_mm^2 + (sigma_rel L)^2); cov_scale >= 0: how much of the two modes' own covariance along the bone widens the
    likelihood; min_length_mm >= 0: two modes nearer than this have no direction, a third of the covariance's trace is used.
    The defaults sigma_mm = 20, sigma_rel = 0, cov_scale = 1 and min_length_mm = 1 are design choices, not measurements: 20 mm
    is a few per cent of a limb and well below the distance between two peaks a heat-map can tell apart (one stride-16 voxel is
    about 130 mm); the modes' covariances are taken at face value; 1 mm is bone_lengths' own floor."""
    s = tuple(scale_mm) if isinstance(scale_mm, (tuple, list, np.ndarray)) else ()
    if len(s) != 3:
        raise ValueError(f'scale_mm must be three numbers (mm per coords01 unit in x, y, z), got {scale_mm!r}')
    p = _lib.MetroSkeletonModes()
    for i, v in enumerate(s):
        p.scale_mm[i] = _finite(f'scale_mm[{i}]', v, 0, False)
    p.sigma_mm = _finite('sigma_mm', sigma_mm, 0, False)
    p.sigma_rel, p.cov_scale = _finite('sigma_rel', sigma_rel, 0, True), _finite('cov_scale', cov_scale, 0, True)
    p.min_length_mm = _finite('min_length_mm', min_length_mm, 0, True)
    return p


def skeleton_edges(edges, n_joints: int) -> np.ndarray:
    """Checks the edges of a skeleton binding: -> int32 [E, 2], E <= 63, output-joint indices in [0, n_joints), no self-edge, no
    cycle (a forest: metro_plan_bind_skeleton_modes refuses anything else, this names the edge first)."""
    e = np.asarray(edges.detach().cpu().numpy() if isinstance(edges, torch.Tensor) else edges)
    if e.size == 0:
        return np.zeros((0, 2), np.int32)
    if e.ndim != 2 or e.shape[1] != 2 or e.dtype.kind not in 'iu' or len(e) > SKELETON_MAX_EDGES:
        raise ValueError(f'edges must be integers [E, 2] with E <= {SKELETON_MAX_EDGES}, got {e.dtype} {e.shape}')
    comp = list(range(n_joints))
    for i, (a, b) in enumerate(e.tolist()):
        if not (0 <= a < n_joints and 0 <= b < n_joints) or a == b:
            raise ValueError(f'edge {i} ({a}, {b}) must join two different joints in [0, {n_joints})')
        if comp[a] == comp[b]:
            raise ValueError(f'edge {i} ({a}, {b}) closes a cycle: the skeleton must be a forest')
        comp = [comp[a] if c == comp[b] else c for c in comp]
    return np.ascontiguousarray(e, np.int32)


def predict_boxes(state: torch.Tensor, ids: torch.Tensor, cameras, frame_sizes, times, coords: str = 'camera', detections=None,
                  detection_frame_index=None, expand: float = 1.25, n_sigma: float = 2.0, max_sigma_mm: float = 300.0,
                  min_joints: Optional[int] = None, max_age_s: float = 1.0, near_mm: float = 100.0, min_side_px: float = 8.0,
                  iou_max: float = 0.3, accel_psd: float = 4e6, clip: bool = True) -> PredictedBoxRows:
    """Next-frame person boxes from the track table, the two launches of metro_predict_boxes on the current stream and no
    synchronisation (include/metro_hip.h has the model).  state float64 [T,J,28] and ids int32 [T] are the table
    associate_tracks walks (frames.new_track_table), on a CUDA device, and are only read.  cameras: the MetroFrameCamera
    table of 1 or F entries (frames.pack_frame_cameras' structured array, uploaded here, or its bytes as a uint8 CUDA tensor
    [n, 240]); frame_sizes int [F,2] (W, H) and times [F] seconds, host values, one per frame, F <= 64.
    coords 'camera' (the state is in each frame's camera; R and t are not read) or 'world'.
    Per (frame, slot): a free slot, or one last seen more than max_age_s before the frame's time, has no box; else every joint
    with a state is advanced to the frame's time by the filter's own prediction (accel_psd as smooth_tracks has it) -- the
    position associate_tracks will compare the next box against -- and projected through the frame's lens-distorted camera.
    A joint counts if it is finite, at least near_mm in front of the camera and inside the monotonic range of the lens model;
    around its pixel it claims a margin of n_sigma standard deviations of its predicted position (at most max_sigma_mm),
    seen at its depth.  The box is the union of those squares, scaled about its centre by expand, cut to the frame (clip),
    and dropped with fewer than min_joints joints (None: (J + 1) // 2) or a side below min_side_px.
    detections float [m,4] (x, y, w, h) with detection_frame_index [m] (None: frame 0), host data or CUDA tensors, m <= 4096:
    a detector's boxes of the same frames, appended after the predicted ones unless their intersection over union with a
    predicted box of their frame reaches iou_max (the tracked person keeps its predicted box) or they are not boxes
    (non-finite, w or h <= 0); suppression among the detections is the detector's own.
    The defaults expand = 1.25, n_sigma = 2, max_sigma_mm = 300, near_mm = 100, min_side_px = 8 and iou_max = 0.3 are
    design choices, not measurements: a quarter more than the joints' extent leaves room for head, hands and feet beyond the outermost joints;
    two standard deviations cover a coasting joint 95 times in 100 per axis; 300 mm keeps a long-unseen track from claiming
    the whole frame; nothing nearer than 100 mm is a person in front of a lens; a crop of fewer than 8 pixels holds no pose;
    two boxes of one person overlap far more than 0.3, two persons side by side less.
    -> PredictedBoxRows, unsliced: counts[0] says how many rows are written, counts[4] > 0 (a detection frame index outside
    [0, F)) is the caller's error to raise.  An empty call (no detections and T F == 0) launches nothing."""
    if coords not in ('camera', 'world'):
        raise ValueError(f"coords must be 'camera' or 'world' (a crop has no calibrated camera to project through), got {coords!r}")
    params, iou = prediction_params(expand, n_sigma, max_sigma_mm, min_joints, max_age_s, near_mm, min_side_px, iou_max, accel_psd)
    if (not isinstance(state, torch.Tensor) or state.dtype != torch.float64 or state.dim() != 3 or state.shape[2] != TRACK_STATE_DOUBLES
            or not 1 <= state.shape[0] <= ASSOC_MAX or not 1 <= state.shape[1] <= _lib.METRO_MAX_JOINTS or not state.is_contiguous()):
        raise ValueError(f'state must be a contiguous float64 tensor [T,J,{TRACK_STATE_DOUBLES}] with 1 <= T <= {ASSOC_MAX} and '
                         f'J <= {_lib.METRO_MAX_JOINTS} (frames.new_track_table)')
    dev, n_tracks, nj = state.device, int(state.shape[0]), int(state.shape[1])
    if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int32 or ids.device != dev or ids.numel() != n_tracks or not ids.is_contiguous():
        raise ValueError(f'ids must be a contiguous int32 tensor of {n_tracks} on {dev} (frames.new_track_table)')
    if min_joints is None:
        min_joints = (nj + 1) // 2
    if min_joints > nj:
        raise ValueError(f'min_joints must be at most the {nj} joints, got {min_joints!r}')
    sizes = np.ascontiguousarray(np.asarray(frame_sizes.cpu() if isinstance(frame_sizes, torch.Tensor) else frame_sizes))
    if sizes.ndim != 2 or sizes.shape[1] != 2 or sizes.dtype.kind not in 'iu' or not 1 <= len(sizes) <= _lib.METRO_MAX_FRAMES:
        raise ValueError(f'frame_sizes must be integers [F, 2] (W, H) with 1 <= F <= {_lib.METRO_MAX_FRAMES} (frames.frame_sizes), got '
                         f'{sizes.dtype} {sizes.shape}')
    if sizes.min() < 1 or sizes.max() > np.iinfo(np.int32).max:
        raise ValueError(f'frame_sizes must be >= 1 pixel, got a frame of {sizes[np.argmin(sizes.min(axis=1))].tolist()}')
    sizes = np.ascontiguousarray(sizes, np.int32)
    n_frames = len(sizes)
    ts = np.ascontiguousarray(np.asarray(times.cpu() if isinstance(times, torch.Tensor) else times, np.float64).reshape(-1))
    if len(ts) != n_frames or not np.isfinite(ts).all():
        raise ValueError(f'times must hold one finite value per frame ({n_frames}), got {len(ts)}')
    if isinstance(cameras, torch.Tensor):
        if cameras.dtype != torch.uint8 or cameras.device != dev or cameras.dim() != 2 or cameras.shape[1] != FRAME_CAMERA_BYTES \
                or not cameras.is_contiguous():
            raise ValueError(f'cameras must be a contiguous uint8 tensor [n, {FRAME_CAMERA_BYTES}] on {dev} (frames.pack_frame_cameras)')
        n_cameras = int(cameras.shape[0])
    else:
        if not isinstance(cameras, np.ndarray) or cameras.dtype.itemsize != FRAME_CAMERA_BYTES or cameras.ndim != 1:
            raise ValueError('cameras must be the structured array frames.pack_frame_cameras returns, or its bytes on the device')
        n_cameras = len(cameras)
    if n_cameras not in (1, n_frames):
        raise ValueError(f'cameras: {n_cameras} entries for {n_frames} frames (one for every frame, or one per frame)')
    det, det_fi, m = None, None, 0
    if detections is not None:
        if isinstance(detections, torch.Tensor) and detections.is_cuda:
            det = detections
        else:
            det = torch.from_numpy(np.ascontiguousarray(np.asarray(detections.cpu() if isinstance(detections, torch.Tensor) else detections,
                                                                   np.float64)))
        if det.dim() != 2 or det.shape[1] != 4 or not det.is_floating_point():
            raise ValueError(f'detections must be floating point [m, 4] (x, y, w, h), got {det.dtype} {tuple(det.shape)}')
        m = int(det.shape[0])
        if m > PREDICT_MAX_DETECTIONS:
            raise ValueError(f'{m} detections: at most {PREDICT_MAX_DETECTIONS} per call')
        if detection_frame_index is None:
            det_fi = torch.zeros(m, dtype=torch.int32)
        else:
            det_fi = detection_frame_index if isinstance(detection_frame_index, torch.Tensor) else \
                torch.from_numpy(np.ascontiguousarray(np.asarray(detection_frame_index).reshape(-1)))
            if det_fi.is_floating_point() or det_fi.is_complex() or det_fi.dtype == torch.bool or det_fi.numel() != m:
                raise ValueError(f'detection_frame_index must hold {m} integers (one per detection), got {det_fi.dtype} '
                                 f'{tuple(det_fi.shape)}')
        if (det.is_cuda and det.device != dev) or (det_fi.is_cuda and det_fi.device != dev):
            raise ValueError(f'detections and detection_frame_index must be host data or on {dev}')
    if dev.type != 'cuda':
        raise ValueError(f'the track table must be on a CUDA device, got {dev}: there is no CPU path')
    from metro_pose3d_amd.frame_formats import _upload
    lib = _lib.load()
    with torch.cuda.device(dev):
        if not isinstance(cameras, torch.Tensor):
            cameras = _upload(np.ascontiguousarray(cameras).view(np.uint8).reshape(n_cameras, FRAME_CAMERA_BYTES), dev)
        if m:
            det = (det if det.is_cuda else det.pin_memory().to(dev, non_blocking=True)).to(torch.float64).contiguous()
            det_fi = det_fi.reshape(-1) if det_fi.is_cuda else det_fi.reshape(-1).pin_memory().to(dev, non_blocking=True)
            if det_fi.dtype != torch.int32:                 # out-of-range values stay out of range through the cast
                det_fi = det_fi.to(torch.int64).clamp(-1, _lib.METRO_MAX_FRAMES).to(torch.int32)
            det_fi = det_fi.contiguous()
        cap = n_frames * n_tracks + m
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        boxes = torch.empty((cap, 4), dtype=torch.float64, device=dev)
        frame, slot, tid, detection, joints = i32(cap), i32(cap), i32(cap), i32(cap), i32(cap)
        dense = torch.empty((n_frames, n_tracks, 4), dtype=torch.float64, device=dev)
        dense_joints, counts = i32(n_frames, n_tracks), i32(5)
        check(lib.metro_predict_boxes(_p(state), _p(ids), n_tracks, nj, _p(cameras), n_cameras, C.c_void_p(sizes.ctypes.data),
                                      C.c_void_p(ts.ctypes.data), n_frames, _COORDS[coords], *params, int(min_joints), int(bool(clip)),
                                      _p(det if m else None), _p(det_fi if m else None), m, iou, _p(dense), _p(dense_joints), _p(boxes),
                                      _p(frame), _p(slot), _p(tid), _p(detection), _p(joints), _p(counts), _stream(dev)),
              'metro_predict_boxes')
    return PredictedBoxRows(boxes, frame, slot, tid, detection, joints, dense, dense_joints, counts)


def backproject_bone_lengths(coords01: torch.Tensor, inv_intrinsics, bone_lengths, spec: ModelSpec,
                             edges: Optional[Sequence[Tuple[int, int]]] = None, root_relative: bool = False,
                             permute: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """coords01 [N,J,3] (head order) + inv_intrinsics [N,3,3] + target bone lengths [E] (dataset means) or [N,E]
    (per pose) -> (coords3d_pred [N,J or Jout,3] mm in camera space, z_offset [N]).  bone_lengths: host values, or a tensor,
    which is used where it is (cast to float64 on the device of coords01): with coords01 and inv_intrinsics on the device too
    the call uploads nothing and does not wait for its stream."""
    lib = _lib.load()
    dev = coords01.device
    c = _f32(coords01, dev, (spec.skeleton.n_head, 3))
    n = c.shape[0]
    k = _f32(torch.as_tensor(inv_intrinsics).reshape(n, 9), dev, (9,))
    e = np.asarray(spec.skeleton.head_edges if edges is None else edges, dtype=np.int32).reshape(-1, 2)
    if e.size == 0 or e.min() < 0 or e.max() >= spec.skeleton.n_head:
        raise ValueError('edges must index head joints')
    te = _table(e, np.int32, dev)
    if isinstance(bone_lengths, torch.Tensor):             # device-resident targets are used where they are: no upload, no wait
        t = bone_lengths.to(device=dev, dtype=torch.float64).contiguous()
    else:
        t = torch.as_tensor(np.asarray(bone_lengths, dtype=np.float64), device=dev).contiguous()
    if t.shape not in ((len(e),), (n, len(e))):
        raise ValueError(f'bone_lengths must be [{len(e)}] or [{n},{len(e)}], got {tuple(t.shape)}')
    cs = spec.to_c(1)
    out = torch.empty((n, spec.skeleton.n_out if permute else spec.skeleton.n_head, 3), dtype=torch.float32, device=dev)
    z = torch.empty((n,), dtype=torch.float32, device=dev)
    check(lib.metro_backproject_bone_lengths(_p(c), _p(k), _p(t), int(t.dim() == 2), _p(te), len(e), n, C.byref(cs),
                                             int(root_relative), int(permute), _p(out), _p(z), _stream(dev)),
          'metro_backproject_bone_lengths')
    return out, z


def backproject_root_depth(coords01: torch.Tensor, inv_intrinsics, root_z, spec: ModelSpec,
                           root_relative: bool = False, permute: bool = False) -> torch.Tensor:
    lib = _lib.load()
    dev = coords01.device
    c = _f32(coords01, dev, (spec.skeleton.n_head, 3))
    n = c.shape[0]
    k = _f32(torch.as_tensor(inv_intrinsics).reshape(n, 9), dev, (9,))
    rz = torch.as_tensor(root_z, dtype=torch.float32, device=dev).contiguous().reshape(n)
    cs = spec.to_c(1)
    out = torch.empty((n, spec.skeleton.n_out if permute else spec.skeleton.n_head, 3), dtype=torch.float32, device=dev)
    check(lib.metro_backproject_root_depth(_p(c), _p(k), _p(rz), n, C.byref(cs), int(root_relative), int(permute), _p(out),
                                           _stream(dev)), 'metro_backproject_root_depth')
    return out


def heatmap_to_25d(coords01: torch.Tensor, spec: ModelSpec) -> torch.Tensor:
    """heatmap_to_25d (volumetric.py:298-300): [N,J,3] in [0,1] -> (x px, y px, z mm), head order."""
    lib = _lib.load()
    dev = coords01.device
    c = _f32(coords01, dev, (spec.skeleton.n_head, 3))
    cs = spec.to_c(1)
    out = torch.empty_like(c)
    check(lib.metro_heatmap_to_25d(_p(c), c.shape[0], C.byref(cs), _p(out), _stream(dev)), 'metro_heatmap_to_25d')
    return out


def to_orig_cam(coords: torch.Tensor, rot_to_orig_cam, mirror_mapping: Sequence[int]) -> torch.Tensor:
    lib = _lib.load()
    dev = coords.device
    x = torch.as_tensor(coords, dtype=torch.float32, device=dev).contiguous()
    n, nj = x.shape[0], x.shape[1]
    r = _f32(torch.as_tensor(rot_to_orig_cam).reshape(n, 9), dev, (9,))
    m = np.asarray(mirror_mapping, dtype=np.int32)
    if m.shape != (nj,) or m.min() < 0 or m.max() >= nj:
        raise ValueError(f'mirror_mapping must be a permutation-like int array of length {nj}')
    tm = _table(m, np.int32, dev)
    out = torch.empty_like(x)
    check(lib.metro_to_orig_cam(_p(x), _p(r), _p(tm), _p(out), n, nj, _stream(dev)), 'metro_to_orig_cam')
    return out
