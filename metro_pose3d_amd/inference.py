"""Drop-in for the reference's `inference.py` (reference inference.py:11-43).

Same call: `estimate_pose(images_tensor, model_path) -> (poses, joint_edges, joint_names)`,
same CLI flag `--model-path`.  Differences that follow from not being TensorFlow:
  * eager: `poses` is a float32 torch.Tensor [N, Jout, 3] (mm, root-relative) on the GPU, already
    computed (the reference returns graph tensors to `sess.run` later, inference.py:25-27);
  * `joint_edges` is an int64 ndarray [E, 2] and `joint_names` an object ndarray of `bytes`,
    which is what `sess.run` yields for those constants (main.py:140-141);
  * `model_path` is a frozen `.pb` GraphDef like the reference's (read without TensorFlow, tfgraph.py) or the
    `.npz` container of modelfile.py;
  * N is free, as with the reference's `[None, 256, 256, 3]` placeholder (main.py:109-111): the call plans for the
    batch it is given -- one `metro_forward` for up to 256 crops, 256-crop chunks beyond.  Kernel dispatch depends on the
    crops per call (tile counts against 256 CUs: from 128 crops on the 3x3 layers take 512-pixel tiles, the head takes
    128- / 256-pixel tiles once it has 256 of them), so results are not bit-stable ACROSS call sizes >= 128 at stride 16
    (estimate_pose docstring);
  * one process per GPU under torch.distributed: the same call shards the batch by image and all-gathers the poses.
Input contract (inference.py:17-18, main.py:109-110): float32 NHWC [N,256,256,3], RGB in [0,1]; or the uint8 RGB bytes such
an image was divided from (byte b = b / 255: the same bits).
The arithmetic mode defaults to fp16, the reference's default compute dtype (options.py:73);
pass precision='f64' (or METRO_PRECISION=f64) for the parity mode (fp64 arithmetic inside).
"""
from __future__ import annotations

import argparse
import contextlib
import os
from collections import OrderedDict
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from metro_pose3d_amd import _lib
from metro_pose3d_amd.engine import Engine
from metro_pose3d_amd.modelfile import load_model

# One plan (workspace sized for its max_batch) per (model file, precision, device, batch bucket), least recently used first.
# Workspace at RN50-s16: 10 MB per crop (2.6 GB at 256 of the 288 GB); the parameter blob (48 MB) is per engine.
BATCH_BUCKETS = (8, 64, 256)
MAX_CACHED_ENGINES = 6
_ENGINES: 'OrderedDict[Tuple[str, float, str, int, int], Engine]' = OrderedDict()


def batch_bucket(n: int) -> int:
    """max_batch of the engine a call with n crops runs on (calls with more than 256 crops are chunked by 256)."""
    for b in BATCH_BUCKETS:
        if n <= b:
            return b
    return BATCH_BUCKETS[-1]


def _engine_for(model_path: str, precision: str, device: torch.device, n: int = 64) -> Engine:
    path = os.path.abspath(model_path)
    key = (path, os.path.getmtime(path), precision, device.index or 0, batch_bucket(n))
    eng = _ENGINES.get(key)
    if eng is None:
        spec, params = load_model(path)
        eng = Engine(spec, params, precision=precision, max_batch=key[-1], device=device)
        _ENGINES[key] = eng
        while len(_ENGINES) > MAX_CACHED_ENGINES:
            _, old = _ENGINES.popitem(last=False)
            old.close()
    else:
        _ENGINES.move_to_end(key)
    return eng


class _ShapeError(ValueError):
    """Wrong image shape: raised identically on every rank of a sharded call, before any collective."""


def clear_cache() -> None:
    """Closes every cached engine (plan, parameter blob, workspace: 2.6 GB at bucket 256) after draining its device."""
    while _ENGINES:
        _, eng = _ENGINES.popitem(last=False)
        eng.close()


def _resolve_device(images_tensor: torch.Tensor) -> torch.device:
    if not torch.cuda.is_available():
        raise _lib.MetroError('no HIP device visible: the MeTRo hot path has no CPU fallback')
    return images_tensor.device if images_tensor.is_cuda else torch.device('cuda', torch.cuda.current_device())


def _gather_shards(local: torch.Tensor, n_total: int, group, status: int = 0):
    """The one collective of the path: all-gather of the per-rank [n_r, Jout, 3] poses with a status row per rank
    (dist.all_gather_poses_with_status).  RCCL moves device tensors (backend `nccl`); any other backend (gloo in the tests) gets
    host tensors and the result goes back.  Returns (poses, status of every rank)."""
    import torch.distributed as dist
    from metro_pose3d_amd.dist import all_gather_poses_with_status
    if dist.get_backend(group) == 'nccl' or not local.is_cuda:
        return all_gather_poses_with_status(local, n_total, status, group)
    out, st = all_gather_poses_with_status(local.cpu(), n_total, status, group)
    return out.to(local.device), st


class PoseUncertainty(NamedTuple):
    """Per-joint confidence read off the heat-maps (estimate_pose(..., return_uncertainty=True)), output joint order."""
    covariance: torch.Tensor     # float32 [n, Jout, 3, 3] mm^2: covariance of each joint's softmax volume
    peak: torch.Tensor           # float32 [n, Jout]: its largest voxel probability, in (0, 1]


class Heatmaps(NamedTuple):
    """Per-joint heat-map marginals (estimate_pose(..., return_heatmaps=True)), output joint order: every joint's softmax
    distribution p over its S x S x D volume, summed over depth and over the image plane."""
    xy: torch.Tensor             # float32 [n, Jout, S, S]: xy[i, r, y, x] = sum_d p[y, x, d]
    z: torch.Tensor              # float32 [n, Jout, D]:    z[i, r, d] = sum_{y,x} p[y, x, d]


def estimate_pose(images_tensor, model_path, precision: Optional[str] = None, check_finite: Optional[bool] = None,
                  shard: Optional[bool] = None, group=None, return_uncertainty: bool = False, return_heatmaps: bool = False):
    """images [N,256,256,3] float32 in [0,1] -> (poses [N,Jout,3] mm, joint_edges, joint_names).

    return_uncertainty=True adds a fourth element, PoseUncertainty(covariance [N,Jout,3,3] mm^2, peak [N,Jout]): every joint's
    output is a softmax distribution over its S x S x D volume and the pose is only its mean; the covariance is that
    distribution's spread (large for an occluded or out-of-crop joint, small for a well-seen one) and peak its largest
    probability.  It is the covariance of the joint's OWN heat-map in the crop's virtual-camera axes, scaled to mm by the linear
    part of heatmap_to_metric -- not the covariance of the root-relative difference the poses are.  Computed by the same
    launches as the poses (metro_forward_moments: the logits never reach HBM), which stay bit for bit those of the plain
    call; sharded calls gather it with the poses in the same collective.

    return_heatmaps=True appends Heatmaps(xy [N,Jout,S,S], z [N,Jout,D]) (after the uncertainty when both are asked): the
    marginals of every joint's softmax volume, the heat-map the reference's net_output_to_heatmap_and_coords returns next to
    the coordinates.  The mean and covariance of a two-peaked joint (left / right confusion, a second person in the crop) say
    only "between" and "wide"; the map shows both peaks.  Written by the same forwards from their own logits
    (metro_plan_bind_heatmaps); the poses and the uncertainty keep their bits, uint8 crops and every precision are served, and
    sharded calls gather the maps with the poses in the same collective.

    uint8 images (RGB bytes, as a JPEG decoder or the crop warp leaves them) are accepted as they are: byte b stands for the
    float32 value b / 255 (normalize01, reference improc.py:56-61) and the result has the bits of the float32 call on those
    values, in every precision.  A quarter of the bytes are uploaded; precision 'f16' reads the bytes in its first kernel
    (metro_forward_u8), the parity precisions expand them on the device first (metro_images_u8_to_f32).

    Multi-GPU (BASELINE.json north star; the reference's call has no such notion): when `torch.distributed` is initialised with
    more than one rank (one process per GPU), EVERY rank makes this same call with the same N images; rank r computes the
    contiguous shard dist.shard_range(N, r, world) on its own GPU and all ranks return the full [N,Jout,3] after ONE all-gather
    of the poses (RCCL over xGMI under backend `nccl`).  No activation crosses ranks, so the result has the bits of the
    single-GPU call as long as both run the same kernel instantiations: at stride 16 always below 128 crops per call (see below).
    `shard=False` keeps the call local; `group` selects a process group.

    Results are NOT bit-stable across call sizes: kernel tile shapes follow the crops per call (the engine buckets of 8 / 64 /
    256; the 3x3 layers take 512-pixel tiles once a layer has 256 of them -- from 128 crops per call at stride 16, 32 at stride 8,
    16 at stride 4; the head takes 128- and then 256-pixel tiles once it has 256 of them: n * S * S / 128 >= 256, i.e. from 128
    crops at stride 16, 32 at stride 8, 8 at stride 4) and every tile shape is another fp32 summation order.  Differences are
    rounding flips of the fp16 chain (tests/test_gpu_forward.py); calls below those sizes agree bit for bit with one another
    whatever their size.

    `check_finite` (default on; METRO_CHECK_FINITE=0 turns it off): the finalize launch's non-finite screen is folded on the
    device after every forward of the call and read back ONCE (one stream synchronisation per call, as the reference's blocking
    sess.run); NonFiniteError is raised when activations overflowed -- a checkpoint whose residual stream exceeds fp16's 65 504
    needs precision='f32m' (or 'f64').  Sharded calls fail COLLECTIVELY: the flag travels in the pose all-gather (one status
    row per rank), so an overflow or an exception on one rank raises on every rank instead of leaving the others blocked in
    the collective.  The screen reads the words of the immediately preceding forward on the engine's workspace and stream: one
    caller per cached engine at a time (an Engine is not thread-safe, like the C plan it wraps)."""
    res = _estimate_pose(images_tensor, model_path, precision, check_finite, shard, group,
                         'placed' if return_uncertainty else None, heatmaps=bool(return_heatmaps))
    return res[:3] + ((res[3],) if return_uncertainty else ()) + ((res[4],) if return_heatmaps else ())


def _estimate_pose(images_tensor, model_path, precision, check_finite, shard, group, uncertainty, heatmaps=False):
    """estimate_pose's body -> (poses, joint_edges, joint_names, uncertainty): None, PoseUncertainty ('placed'), or, for the
    frames chain, which rotates and averages them itself, the forward's own (cov01 [N,J_head,6], peak [N,J_head]) ('head':
    local calls only).  `heatmaps`: a fifth element, Heatmaps."""
    if precision is None:
        precision = os.environ.get('METRO_PRECISION', 'f16')
    if check_finite is None:
        check_finite = os.environ.get('METRO_CHECK_FINITE', '1') != '0'
    if isinstance(images_tensor, np.ndarray):
        images_tensor = torch.from_numpy(images_tensor)
    if not isinstance(images_tensor, torch.Tensor):
        raise ValueError(f'images must be a torch.Tensor or numpy array, got {type(images_tensor)}')
    if images_tensor.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f'images must be float32 in [0,1] (reference inference.py:18) or uint8 RGB bytes, got {images_tensor.dtype}')
    device = _resolve_device(images_tensor)
    n = int(images_tensor.shape[0]) if images_tensor.dim() == 4 else 0
    rank, world = 0, 1
    if shard is not False:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            rank, world = dist.get_rank(group), dist.get_world_size(group)
        elif shard:
            raise _lib.MetroError('shard=True needs an initialised torch.distributed process group with more than one rank')
    from metro_pose3d_amd.dist import shard_range
    begin, end = shard_range(n, rank, world) if n else (0, 0)
    # Per-rank failures must not leave the other ranks blocked in the gather: a failing rank records its error, STILL joins the
    # collective (its status row says so) and every rank raises afterwards.  Status: 0 fine, k > 0 = k crops of this rank's
    # shard reached the soft-argmax non-finite (fp16 overflow), -1 = this rank raised -- in the model load, the plan build, the
    # workspace allocation, the shard upload or the forward loop (all inside the try since round 6).
    # What is NOT covered: a failure that leaves this rank unable to take part in a collective at all -- the model file cannot be
    # read far enough to learn the output joint count (every rank passes the same path: they then all raise here, before any
    # collective), a wrong image shape (ValueError on every rank alike), or a sticky HIP error after which no device tensor can
    # be allocated under backend `nccl` (the process group's own timeout ends the other ranks).
    status, err, eng, poses, n_out = 0, None, None, None, None
    cov01 = peak = heat_xy = heat_z = None
    width = 13 if uncertainty == 'placed' else 3          # gathered row: pose (3) + covariance (9) + peak (1) [+ xy (S * S) + z (D)]
    heat_dims = None                                      # (S, D) once the spec is known
    with (torch.cuda.device(device) if device.type == 'cuda' else contextlib.nullcontext()):
        try:
            eng = _engine_for(model_path, precision, device, max(end - begin, 1))
            s = eng.spec.proc_side
            n_out = eng.spec.skeleton.n_out
            heat_dims = (eng.spec.heatmap_side, eng.spec.depth)
            if images_tensor.dim() != 4 or tuple(images_tensor.shape[1:]) != (s, s, 3):
                raise _ShapeError(f'images must be NHWC [N,{s},{s},3] (reference main.py:109-110), got '
                                  f'{tuple(images_tensor.shape)}')
            images = images_tensor[begin:end].to(device, non_blocking=True).contiguous()      # only this rank's shard goes to its GPU
            poses = torch.empty((end - begin, n_out, 3), dtype=torch.float32, device=device)
            if uncertainty:
                cov01 = torch.empty((end - begin, eng.spec.skeleton.n_head, 6), dtype=torch.float32, device=device)
                peak = torch.empty((end - begin, eng.spec.skeleton.n_head), dtype=torch.float32, device=device)
            if heatmaps:
                xy_shape, z_shape = eng.heat_shapes(end - begin)
                heat_xy = torch.empty(xy_shape, dtype=torch.float32, device=device)
                heat_z = torch.empty(z_shape, dtype=torch.float32, device=device)
            bad = None
            for i in range(0, end - begin, eng.max_batch):
                k = min(eng.max_batch, end - begin - i)
                kw = dict(cov01=cov01[i:i + k], peak=peak[i:i + k]) if uncertainty else {}
                if heatmaps:
                    kw.update(heat_xy=heat_xy[i:i + k], heat_z=heat_z[i:i + k])
                eng.forward(images[i:i + k], out=poses[i:i + k], **kw)
                if check_finite:       # folded on the device after every chunk: ONE synchronisation per call, below
                    cnt = eng.status_words(k).ne(0).sum()
                    bad = cnt if bad is None else bad + cnt
            if uncertainty == 'placed':
                from metro_pose3d_amd.heads import place_covariances
                if end > begin:
                    cov, pk = place_covariances(cov01, peak, eng.spec)
                else:
                    cov, pk = poses.new_empty((0, n_out, 3, 3)), poses.new_empty((0, n_out))
                poses = torch.cat([poses, cov.reshape(-1, n_out, 9), pk[..., None]], dim=2)
            if heatmaps:
                poses = torch.cat([poses, heat_xy.reshape(end - begin, n_out, heat_dims[0] ** 2), heat_z], dim=2)
            if bad is not None:
                status = int(bad.item())                                 # the call's one stream synchronisation
        except _ShapeError:
            raise                       # the same on every rank (same images): no collective was entered by anybody
        except Exception as e:          # noqa: BLE001 -- re-raised below, after the collective
            status, err = -1, e
        if world > 1:
            try:
                if err is not None:
                    # join with a FRESH tensor that only carries the status row: `poses` may be unallocated or hold garbage
                    if n_out is None:
                        spec = load_model(model_path)[0]                        # raises if the file is unreadable (every rank alike)
                        n_out, heat_dims = spec.skeleton.n_out, (spec.heatmap_side, spec.depth)
                    if heatmaps:
                        width += heat_dims[0] * heat_dims[0] + heat_dims[1]
                    on_host = torch.distributed.get_backend(group) != 'nccl'
                    poses = torch.zeros((end - begin, n_out, width), dtype=torch.float32, device='cpu' if on_host else device)
                poses, statuses = _gather_shards(poses, n, group, status)
            except Exception:
                if err is not None:
                    raise err
                raise
        else:
            statuses = [status]
    if err is not None:
        raise err
    if any(st != 0 for st in statuses):
        failed = ', '.join(f'rank {r}: ' + ('raised (model load, plan build, upload or forward)' if st < 0 else f'{st} crops') for r, st in enumerate(statuses) if st != 0)
        if any(st < 0 for st in statuses):
            raise _lib.MetroError(f'estimate_pose failed on another rank ({failed}); no poses returned on any rank')
        raise _lib.NonFiniteError(
            f'{eng.spec.arch_name} stride {eng.spec.stride} in precision {precision!r}: crops reached the soft-argmax with non-finite '
            f'statistics ({failed})' + (' (fp16 storage overflows at 65504: run this model with precision f32m or f64)' if precision == 'f16' else ''))
    sk = eng.spec.skeleton
    names = np.empty(sk.n_out, dtype=object)
    names[:] = sk.names_bytes()
    heat = None
    if heatmaps:
        side, depth = heat_dims
        base = 13 if uncertainty == 'placed' else 3
        heat = Heatmaps(poses[..., base:base + side * side].reshape(-1, sk.n_out, side, side).contiguous(),
                        poses[..., base + side * side:].contiguous())
        poses = poses[..., :base]
    unc = None
    if uncertainty == 'placed':
        unc = PoseUncertainty(poses[..., 3:12].reshape(-1, sk.n_out, 3, 3).contiguous(), poses[..., 12].contiguous())
        poses = poses[..., :3].contiguous()
    elif uncertainty == 'head':
        unc = (cov01, peak)
    if heatmaps:
        return poses.contiguous(), sk.edges_array(), names, unc, heat
    return poses, sk.edges_array(), names, unc


class Modes(NamedTuple):
    """Per-joint heat-map modes (estimate_pose_modes), output joint order: the K places a joint may be, how much probability
    each holds and how tight each is.  A missing mode (fewer than K local maxima far enough apart) has voxel -1, mass 0 and NaN
    elsewhere; a joint with a NaN or +Inf logit has voxel -1 and NaN everywhere."""
    poses: torch.Tensor          # float32 [n, Jout, K, 3] mm, in the frame of the call's own poses (relative to the root's MEAN)
    covariance: torch.Tensor     # float32 [n, Jout, K, 3, 3] mm^2: of the joint's softmax over the mode's window, about its mean
    mass: torch.Tensor           # float32 [n, Jout, K]: the probability inside the window; a joint's masses sum to at most 1
    peak: torch.Tensor           # float32 [n, Jout, K]: the probability of the mode's own voxel
    voxel: torch.Tensor          # int32 [n, Jout, K]: its linear index (y * S + x) * D + d, or -1


def modes_to_metric(spec, stats: torch.Tensor, coords01: torch.Tensor, voxel: torch.Tensor) -> Modes:
    """Engine.forward_modes' stats [n, Jout, K, 11] and voxel, and the same call's coords01 [n, J_head, 3] -> Modes.  Positions:
    heatmap_to_metric (reference volumetric.py:288-306) of the mode's coords01 minus that of the root joint's mean (the last head
    joint, tfu3d.py:23-25), so the plain pose is the mass-weighted blend of a joint's modes when they hold all the mass.
    Covariances: diag(s) Cov01 diag(s) with the linear part of heatmap_to_metric, the scaling of
    heads.place_covariances(..., coords='crop').  fp64 arithmetic on the fp32 inputs, one rounding per output."""
    from metro_pose3d_amd.heads import cov6_to_3x3
    last = spec.proc_side - 1
    lrc, half = float(last - last % spec.stride - 1), float(spec.stride // 2)
    box, side = float(spec.box_size_mm), float(spec.proc_side)

    def metric(c):
        return torch.cat([(c[..., :2] * lrc + half) * box / side, c[..., 2:] * box], dim=-1)
    st = stats.double()
    root = metric(coords01.double()[:, -1])                                                # [n, 3]
    s = torch.tensor([lrc * box / side, lrc * box / side, box], dtype=torch.float64, device=stats.device)
    cov = cov6_to_3x3(st[..., 5:]) * (s[:, None] * s[None, :])
    return Modes((metric(st[..., 2:5]) - root[:, None, None, :]).float(), cov.float(), stats[..., 0].contiguous(),
                 stats[..., 1].contiguous(), voxel)


def estimate_pose_modes(images_tensor, model_path, k: int = 2, radius: int = 1, precision: Optional[str] = None,
                        check_finite: Optional[bool] = None, return_uncertainty: bool = False, return_heatmaps: bool = False,
                        *, shard: Optional[bool] = None):
    """estimate_pose that also returns every joint's heat-map modes: estimate_pose's tuple (with the PoseUncertainty and the
    Heatmaps where asked), and Modes appended last.  For a two-peaked joint (left / right confusion, a second person in the
    crop) the pose lies between the peaks and at neither; the modes are the k places the joint may be -- local maxima of its
    logits, none within 2 * radius voxels of another -- each with its probability mass, position and covariance over the window
    of `radius` voxels around it (metro_plan_bind_modes; Engine.forward_modes).  Written by the same forwards from their own
    logits; poses, uncertainty and heat-maps keep the bits estimate_pose gives them; uint8 crops and every precision are
    served.  A local call: sharded calls do not return modes (shard=True raises ValueError)."""
    if shard:
        raise ValueError('estimate_pose_modes: sharded calls do not return modes (shard must be None or False)')
    for name, v, hi in (('k', k, _lib.METRO_MAX_MODES), ('radius', radius, _lib.METRO_MAX_MODE_RADIUS)):
        if isinstance(v, bool) or not isinstance(v, int) or not (1 if name == 'k' else 0) <= v <= hi:
            raise ValueError(f'{name} must be an int in [{1 if name == "k" else 0}, {hi}], got {v!r}')
    if precision is None:
        precision = os.environ.get('METRO_PRECISION', 'f16')
    if check_finite is None:
        check_finite = os.environ.get('METRO_CHECK_FINITE', '1') != '0'
    if isinstance(images_tensor, np.ndarray):
        images_tensor = torch.from_numpy(images_tensor)
    if not isinstance(images_tensor, torch.Tensor):
        raise ValueError(f'images must be a torch.Tensor or numpy array, got {type(images_tensor)}')
    if images_tensor.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f'images must be float32 in [0,1] (reference inference.py:18) or uint8 RGB bytes, got {images_tensor.dtype}')
    device = _resolve_device(images_tensor)
    n = int(images_tensor.shape[0]) if images_tensor.dim() == 4 else 0
    with torch.cuda.device(device):
        eng = _engine_for(model_path, precision, device, max(n, 1))
        sk, s = eng.spec.skeleton, eng.spec.proc_side
        if images_tensor.dim() != 4 or tuple(images_tensor.shape[1:]) != (s, s, 3):
            raise _ShapeError(f'images must be NHWC [N,{s},{s},3] (reference main.py:109-110), got {tuple(images_tensor.shape)}')
        images = images_tensor.to(device, non_blocking=True).contiguous()
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)
        poses, coords01 = f32(n, sk.n_out, 3), f32(n, sk.n_head, 3)
        cov01, peak = (f32(n, sk.n_head, 6), f32(n, sk.n_head)) if return_uncertainty else (None, None)
        heat_xy, heat_z = (f32(*eng.heat_shapes(n)[0]), f32(*eng.heat_shapes(n)[1])) if return_heatmaps else (None, None)
        part = lambda t, i, m: None if t is None else t[i:i + m]
        voxels, stats, bad = [], [], None
        for i in range(0, n, eng.max_batch):
            m = min(eng.max_batch, n - i)
            _, vx, st = eng.forward_modes(images[i:i + m], k, radius, poses[i:i + m], coords01[i:i + m], part(cov01, i, m),
                                          part(peak, i, m), part(heat_xy, i, m), part(heat_z, i, m))
            voxels.append(vx)
            stats.append(st)
            if check_finite:       # folded on the device after every chunk: one synchronisation per call, below
                cnt = eng.status_words(m).ne(0).sum()
                bad = cnt if bad is None else bad + cnt
        if bad is not None and int(bad.item()):
            raise _lib.NonFiniteError(
                f'{eng.spec.arch_name} stride {eng.spec.stride} in precision {precision!r}: {int(bad.item())} crops reached the '
                f'soft-argmax with non-finite statistics' +
                (' (fp16 storage overflows at 65504: run this model with precision f32m or f64)' if precision == 'f16' else ''))
        res = [poses, sk.edges_array(), None]
        names = np.empty(sk.n_out, dtype=object)
        names[:] = sk.names_bytes()
        res[2] = names
        if return_uncertainty:
            from metro_pose3d_amd.heads import place_covariances
            res.append(PoseUncertainty(*place_covariances(cov01, peak, eng.spec)) if n else
                       PoseUncertainty(poses.new_empty((0, sk.n_out, 3, 3)), poses.new_empty((0, sk.n_out))))
        if return_heatmaps:
            res.append(Heatmaps(heat_xy, heat_z))
        vx = torch.cat(voxels) if voxels else torch.empty((0, sk.n_out, k), dtype=torch.int32, device=device)
        st = torch.cat(stats) if stats else f32(0, sk.n_out, k, Engine.MODE_STATS)
        res.append(modes_to_metric(eng.spec, st, coords01, vx))
    return tuple(res)


class SkeletonModes(NamedTuple):
    """The choice among every joint's heat-map modes by the person's bone lengths (estimate_pose_skeleton), output joint order.
    A joint without a usable mode (a NaN or +Inf logit) has choice -1, NaN in prob and both logs, and keeps its plain pose."""
    poses: torch.Tensor          # float32 [n, Jout, 3] mm: the chosen modes' positions minus the chosen root's
    choice: torch.Tensor         # int32 [n, Jout]: the joint's mode in the most probable assignment of the whole skeleton
    prob: torch.Tensor           # float32 [n, Jout, K]: the marginal probability of every mode under the skeleton
    log_evidence: torch.Tensor   # float32 [n, Jout]: ln of the probability the modes give to the bone lengths (<= 0), per component
    log_map: torch.Tensor        # float32 [n, Jout]: ln of the probability of the chosen assignment of the joint's component


def skeleton_to_metric(spec, coords01_sel: torch.Tensor) -> torch.Tensor:
    """Engine.forward_skeleton_modes' coords01_sel [n, J_head, 3] -> the selected poses float32 [n, Jout, 3] in mm:
    heatmap_to_metric (reference volumetric.py:288-306) of the chosen modes' means minus that of the root -- the chosen root
    where the output order carries the root head joint (the last one, tfu3d.py:23-25), else its plain mean, which coords01_sel
    holds there (posterior_to_metric's rule).  fp64 arithmetic on the fp32 input, one rounding per output."""
    sk = spec.skeleton
    a, b = _metric_map(spec)
    a = torch.tensor(a, dtype=torch.float64, device=coords01_sel.device)
    b = torch.tensor(b, dtype=torch.float64, device=coords01_sel.device)
    if coords01_sel.dim() != 3 or tuple(coords01_sel.shape[1:]) != (sk.n_head, 3):
        raise ValueError(f'coords01_sel must be [n, {sk.n_head}, 3], got {tuple(coords01_sel.shape)}')
    positions = coords01_sel.double() * a + b
    perm = torch.tensor(list(sk.permutation), dtype=torch.int64, device=coords01_sel.device)
    return (positions[:, perm] - positions[:, -1:]).float()


def _bone_length_rows(bone_lengths, n: int, n_edges: int, device) -> torch.Tensor:
    """bone_lengths [E] or [n, E], NumPy or tensor, mm -> float64 [n, E] on `device`, contiguous.  The values are not read: NaN
    (or <= 0) is the caller's way to say that a bone is unknown."""
    t = torch.from_numpy(np.asarray(bone_lengths)) if not isinstance(bone_lengths, torch.Tensor) else bone_lengths
    if t.dtype.is_complex or t.dtype == torch.bool or t.dim() not in (1, 2) or t.shape[-1] != n_edges or (t.dim() == 2 and t.shape[0] != n):
        raise ValueError(f'bone_lengths must be numbers [{n_edges}] or [{n}, {n_edges}] (mm, in skeleton.edges order; NaN: unknown), got '
                         f'{t.dtype} {tuple(t.shape)}')
    t = t.to(device=device, dtype=torch.float64, non_blocking=True)
    return (t[None].expand(n, n_edges) if t.dim() == 1 else t).contiguous()


def estimate_pose_skeleton(images_tensor, model_path, bone_lengths, k: int = 2, radius: int = 1, sigma_mm: float = 20.0,
                           sigma_rel: float = 0.0, cov_scale: float = 1.0, min_length_mm: float = 1.0,
                           precision: Optional[str] = None, check_finite: Optional[bool] = None, return_uncertainty: bool = False,
                           return_heatmaps: bool = False, *, shard: Optional[bool] = None):
    """estimate_pose_modes that also chooses among every joint's modes by the person's bone lengths: estimate_pose's tuple (with
    the PoseUncertainty and the Heatmaps where asked), then Modes, then SkeletonModes.  A wrist's heat-map with two peaks (a
    left / right swap, a second person in the crop) has its mean between them and its heavier peak may be the wrong one; only
    one of the two is a forearm's length from the elbow.  bone_lengths: [E] or [n, E] in mm, NumPy or tensor, in skeleton.edges
    order (a person's own: Follower.bone_lengths_for; NaN: that bone is unknown).  The skeleton is a tree, so the most probable
    assignment of a mode to every joint and every mode's marginal are exact, one small launch per forward behind the modes'
    (metro_plan_bind_skeleton_modes; Engine.forward_skeleton_modes, which holds the other keywords).  It can only choose among
    the modes found, and lengths are compared in MeTRo's metric scale.  Poses, uncertainty, heat-maps and modes keep the bits
    estimate_pose_modes gives them; uint8 crops and every precision are served.  A local call: shard=True raises ValueError."""
    if shard:
        raise ValueError('estimate_pose_skeleton: sharded calls do not choose modes (shard must be None or False)')
    if precision is None:
        precision = os.environ.get('METRO_PRECISION', 'f16')
    if check_finite is None:
        check_finite = os.environ.get('METRO_CHECK_FINITE', '1') != '0'
    if isinstance(images_tensor, np.ndarray):
        images_tensor = torch.from_numpy(images_tensor)
    if not isinstance(images_tensor, torch.Tensor):
        raise ValueError(f'images must be a torch.Tensor or numpy array, got {type(images_tensor)}')
    if images_tensor.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f'images must be float32 in [0,1] (reference inference.py:18) or uint8 RGB bytes, got {images_tensor.dtype}')
    device = _resolve_device(images_tensor)
    n = int(images_tensor.shape[0]) if images_tensor.dim() == 4 else 0
    with torch.cuda.device(device):
        eng = _engine_for(model_path, precision, device, max(n, 1))
        sk, s = eng.spec.skeleton, eng.spec.proc_side
        if images_tensor.dim() != 4 or tuple(images_tensor.shape[1:]) != (s, s, 3):
            raise _ShapeError(f'images must be NHWC [N,{s},{s},3] (reference main.py:109-110), got {tuple(images_tensor.shape)}')
        lengths = _bone_length_rows(bone_lengths, n, len(sk.edges), device)
        images = images_tensor.to(device, non_blocking=True).contiguous()
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)
        poses, coords01 = f32(n, sk.n_out, 3), f32(n, sk.n_head, 3)
        cov01, peak = (f32(n, sk.n_head, 6), f32(n, sk.n_head)) if return_uncertainty else (None, None)
        heat_xy, heat_z = (f32(*eng.heat_shapes(n)[0]), f32(*eng.heat_shapes(n)[1])) if return_heatmaps else (None, None)
        part = lambda t, i, m: None if t is None else t[i:i + m]
        parts, bad = [], None
        for i in range(0, n, eng.max_batch):
            m = min(eng.max_batch, n - i)
            parts.append(eng.forward_skeleton_modes(images[i:i + m], lengths[i:i + m], k, radius, None, sigma_mm, sigma_rel, cov_scale,
                                                    min_length_mm, poses[i:i + m], coords01[i:i + m], part(cov01, i, m),
                                                    part(peak, i, m), part(heat_xy, i, m), part(heat_z, i, m))[1:])
            if check_finite:       # folded on the device after every chunk: one synchronisation per call, below
                cnt = eng.status_words(m).ne(0).sum()
                bad = cnt if bad is None else bad + cnt
        if bad is not None and int(bad.item()):
            raise _lib.NonFiniteError(
                f'{eng.spec.arch_name} stride {eng.spec.stride} in precision {precision!r}: {int(bad.item())} crops reached the '
                f'soft-argmax with non-finite statistics' +
                (' (fp16 storage overflows at 65504: run this model with precision f32m or f64)' if precision == 'f16' else ''))
        names = np.empty(sk.n_out, dtype=object)
        names[:] = sk.names_bytes()
        res = [poses, sk.edges_array(), names]
        if return_uncertainty:
            from metro_pose3d_amd.heads import place_covariances
            res.append(PoseUncertainty(*place_covariances(cov01, peak, eng.spec)) if n else
                       PoseUncertainty(poses.new_empty((0, sk.n_out, 3, 3)), poses.new_empty((0, sk.n_out))))
        if return_heatmaps:
            res.append(Heatmaps(heat_xy, heat_z))
        if parts:
            vx, st, choice, prob, info, sel = (torch.cat(t) for t in zip(*parts))
        else:
            vx, choice = (torch.empty(sh, dtype=torch.int32, device=device) for sh in ((0, sk.n_out, k), (0, sk.n_out)))
            st, prob, info, sel = f32(0, sk.n_out, k, Engine.MODE_STATS), f32(0, sk.n_out, k), f32(0, sk.n_out, 2), f32(0, sk.n_head, 3)
        res.append(modes_to_metric(eng.spec, st, coords01, vx))
        res.append(SkeletonModes(skeleton_to_metric(eng.spec, sel), choice, prob, info[..., 0].contiguous(), info[..., 1].contiguous()))
    return tuple(res)


class Posterior(NamedTuple):
    """Per-joint heat-map posterior under a Gaussian prior (estimate_pose_posterior), output joint order: the joint's softmax
    times the prior, over the whole volume.  A joint with a NaN in its prior row or a NaN / +Inf logit is NaN everywhere."""
    poses: torch.Tensor          # float32 [n, Jout, 3] mm: `positions` minus the posterior root's position
    positions: torch.Tensor      # float32 [n, Jout, 3] mm: heatmap_to_metric of the posterior mean, un-rooted (crop-metric frame)
    covariance: torch.Tensor     # float32 [n, Jout, 3, 3] mm^2: of the posterior, about its mean
    log_evidence: torch.Tensor   # float32 [n, Jout]: ln of the probability the heat-map gives to the prior's region (<= 0)
    peak: torch.Tensor           # float32 [n, Jout]: the largest posterior probability of a voxel


def _metric_map(spec):
    """heatmap_to_metric (reference volumetric.py:288-306) as mm = a * coords01 + b per axis: (a [3], b [3]), Python floats."""
    last = spec.proc_side - 1
    lrc, half = float(last - last % spec.stride - 1), float(spec.stride // 2)
    box, side = float(spec.box_size_mm), float(spec.proc_side)
    return (lrc * box / side, lrc * box / side, box), (half * box / side, half * box / side, 0.0)


def _check_prior_arrays(positions, precision, n=None):
    """Shapes and dtypes of a prior in mm: positions [n, Jout, 3] and precision [n, Jout, 3, 3], both NumPy arrays or both torch
    tensors of a float type; HOST arrays are also checked for symmetry and for being positive semi-definite (CUDA tensors are
    not read).  -> (positions, precision) as float64 torch tensors on the inputs' device."""
    if isinstance(positions, np.ndarray):
        positions = torch.from_numpy(positions)
    if isinstance(precision, np.ndarray):
        precision = torch.from_numpy(precision)
    for name, t in (('prior positions', positions), ('prior precision', precision)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f'{name} must be a torch.Tensor or numpy array, got {type(t)}')
        if not t.dtype.is_floating_point:
            raise ValueError(f'{name} must be of a float type, got {t.dtype}')
    if positions.dim() != 3 or positions.shape[-1] != 3:
        raise ValueError(f'prior positions must be [n, Jout, 3] (mm), got {tuple(positions.shape)}')
    if tuple(precision.shape) != tuple(positions.shape) + (3,):
        raise ValueError(f'prior precision must be {tuple(positions.shape) + (3,)} (1/mm^2, one symmetric 3 x 3 matrix per joint), '
                         f'got {tuple(precision.shape)}')
    if n is not None and positions.shape[0] != n:
        raise ValueError(f'the prior holds {positions.shape[0]} crops, the images {n}')
    if precision.device != positions.device:
        raise ValueError(f'prior positions are on {positions.device}, the precision on {precision.device}')
    positions, precision = positions.double(), precision.double()
    if not precision.is_cuda and precision.numel():
        lam = precision.numpy()
        ok = np.isfinite(lam).all(axis=(-1, -2))          # a NaN row is the caller's way to poison a joint: passed on
        size = np.abs(lam).max(axis=(-1, -2), initial=0.0)
        skew = np.abs(lam - np.swapaxes(lam, -1, -2)).max(axis=(-1, -2))
        if (ok & (skew > 1e-9 * size)).any():
            i = np.argwhere(ok & (skew > 1e-9 * size))[0]
            raise ValueError(f'prior precision of crop {i[0]}, joint {i[1]} is not symmetric')
        low = np.linalg.eigvalsh(np.where(ok[..., None, None], 0.5 * (lam + np.swapaxes(lam, -1, -2)), 0.0))[..., 0]
        if (low < -1e-9 * size).any():
            i = np.argwhere(low < -1e-9 * size)[0]
            raise ValueError(f'prior precision of crop {i[0]}, joint {i[1]} is not positive semi-definite (lowest eigenvalue {low[tuple(i)]:g})')
    return positions, precision


def pose_prior(spec, positions_mm, precision_mm) -> torch.Tensor:
    """A Gaussian prior in mm -> the prior rows Engine.forward_posterior takes, float32 [n, Jout, 9] on the inputs' device:
    positions_mm [n, Jout, 3] in the crop-metric frame of Posterior.positions (un-rooted), precision_mm [n, Jout, 3, 3] in
    1/mm^2 (symmetric positive semi-definite; singular and zero matrices are fine: no knowledge along those axes).  The inverse
    of the linear map of posterior_to_metric: mu = (mm - b) / a per axis and L01 = diag(a) Lmm diag(a), words (xx, yy, zz, xy,
    xz, yz).  fp64 arithmetic, one rounding per value.  Host arrays are checked for symmetry and definiteness; CUDA tensors
    are not read."""
    pos, lam = _check_prior_arrays(positions_mm, precision_mm)
    a, b = _metric_map(spec)
    a = torch.tensor(a, dtype=torch.float64, device=pos.device)
    b = torch.tensor(b, dtype=torch.float64, device=pos.device)
    mu = (pos - b) / a
    l01 = lam * (a[:, None] * a[None, :])
    words = [l01[..., 0, 0], l01[..., 1, 1], l01[..., 2, 2], l01[..., 0, 1], l01[..., 0, 2], l01[..., 1, 2]]
    return torch.cat([mu, torch.stack(words, -1)], -1).float().contiguous()


def posterior_to_metric(spec, post: torch.Tensor, coords01: Optional[torch.Tensor] = None) -> Posterior:
    """Engine.forward_posterior's post [n, Jout, 11] -> Posterior.  Positions: heatmap_to_metric (reference volumetric.py:288-306)
    of the posterior mean.  Poses: positions minus the posterior root's -- the output row of the root head joint (the last head
    joint, tfu3d.py:23-25); a skeleton whose output order does not carry it (the merged one) takes the root's plain mean from the
    same call's coords01 [n, J_head, 3], which must then be given.  Covariances: diag(a) Cov01 diag(a), the scaling of
    modes_to_metric.  fp64 arithmetic on the fp32 inputs, one rounding per output."""
    from metro_pose3d_amd.heads import cov6_to_3x3
    sk = spec.skeleton
    a, b = _metric_map(spec)
    a = torch.tensor(a, dtype=torch.float64, device=post.device)
    b = torch.tensor(b, dtype=torch.float64, device=post.device)
    if post.dim() != 3 or tuple(post.shape[1:]) != (sk.n_out, Engine.POST_STATS):
        raise ValueError(f'post must be [n, {sk.n_out}, {Engine.POST_STATS}], got {tuple(post.shape)}')
    pd = post.double()
    positions = pd[..., 2:5] * a + b
    perm = list(sk.permutation)
    if sk.n_head - 1 in perm:
        root = positions[:, perm.index(sk.n_head - 1)]
    elif coords01 is not None:
        root = coords01.double()[:, -1] * a + b
    else:
        raise ValueError('the output joints of this skeleton do not carry the root head joint: pass the same call\'s coords01')
    cov = cov6_to_3x3(pd[..., 5:]) * (a[:, None] * a[None, :])
    return Posterior((positions - root[:, None, :]).float(), positions.float(), cov.float(), post[..., 0].contiguous(),
                     post[..., 1].contiguous())


def estimate_pose_posterior(images_tensor, model_path, prior_positions, prior_precision, precision: Optional[str] = None,
                            check_finite: Optional[bool] = None, return_uncertainty: bool = False, return_heatmaps: bool = False,
                            *, shard: Optional[bool] = None):
    """estimate_pose that also returns every joint's heat-map posterior under a Gaussian prior: estimate_pose's tuple (with the
    PoseUncertainty and the Heatmaps where asked), and Posterior appended last.  The prior is what the caller already knows -- a
    tracker's prediction, the previous frame's pose: prior_positions [n, Jout, 3] in mm, in the crop-metric frame of
    Posterior.positions, and prior_precision [n, Jout, 3, 3] in 1/mm^2 (positive semi-definite; a zero row and column: no
    knowledge along that axis; see pose_prior).  For a two-peaked joint the plain pose lies between the peaks; the posterior
    mean is taken from the peak that agrees with the prior, its covariance is that peak's, and exp(log_evidence) is the
    probability the heat-map gives to the prior's region (metro_plan_bind_prior; Engine.forward_posterior).  Written by the same
    forwards from their own logits; poses, uncertainty and heat-maps keep the bits estimate_pose gives them; uint8 crops and
    every precision are served.  A local call: sharded calls do not return posteriors (shard=True raises ValueError)."""
    if shard:
        raise ValueError('estimate_pose_posterior: sharded calls do not return posteriors (shard must be None or False)')
    if precision is None:
        precision = os.environ.get('METRO_PRECISION', 'f16')
    if check_finite is None:
        check_finite = os.environ.get('METRO_CHECK_FINITE', '1') != '0'
    if isinstance(images_tensor, np.ndarray):
        images_tensor = torch.from_numpy(images_tensor)
    if not isinstance(images_tensor, torch.Tensor):
        raise ValueError(f'images must be a torch.Tensor or numpy array, got {type(images_tensor)}')
    if images_tensor.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f'images must be float32 in [0,1] (reference inference.py:18) or uint8 RGB bytes, got {images_tensor.dtype}')
    n = int(images_tensor.shape[0]) if images_tensor.dim() == 4 else 0
    _check_prior_arrays(prior_positions, prior_precision, n if images_tensor.dim() == 4 else None)
    device = _resolve_device(images_tensor)
    with torch.cuda.device(device):
        eng = _engine_for(model_path, precision, device, max(n, 1))
        sk, s = eng.spec.skeleton, eng.spec.proc_side
        if images_tensor.dim() != 4 or tuple(images_tensor.shape[1:]) != (s, s, 3):
            raise _ShapeError(f'images must be NHWC [N,{s},{s},3] (reference main.py:109-110), got {tuple(images_tensor.shape)}')
        prior = pose_prior(eng.spec, prior_positions, prior_precision)
        if prior.shape[1] != sk.n_out:
            raise ValueError(f'the prior holds {prior.shape[1]} joints, the model returns {sk.n_out}')
        prior = prior.to(device, non_blocking=True)
        images = images_tensor.to(device, non_blocking=True).contiguous()
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)
        poses, coords01 = f32(n, sk.n_out, 3), f32(n, sk.n_head, 3)
        cov01, peak = (f32(n, sk.n_head, 6), f32(n, sk.n_head)) if return_uncertainty else (None, None)
        heat_xy, heat_z = (f32(*eng.heat_shapes(n)[0]), f32(*eng.heat_shapes(n)[1])) if return_heatmaps else (None, None)
        part = lambda t, i, m: None if t is None else t[i:i + m]
        posts, bad = [], None
        for i in range(0, n, eng.max_batch):
            m = min(eng.max_batch, n - i)
            _, po = eng.forward_posterior(images[i:i + m], prior[i:i + m], poses[i:i + m], coords01[i:i + m], part(cov01, i, m),
                                          part(peak, i, m), part(heat_xy, i, m), part(heat_z, i, m))
            posts.append(po)
            if check_finite:       # folded on the device after every chunk: one synchronisation per call, below
                cnt = eng.status_words(m).ne(0).sum()
                bad = cnt if bad is None else bad + cnt
        if bad is not None and int(bad.item()):
            raise _lib.NonFiniteError(
                f'{eng.spec.arch_name} stride {eng.spec.stride} in precision {precision!r}: {int(bad.item())} crops reached the '
                f'soft-argmax with non-finite statistics' +
                (' (fp16 storage overflows at 65504: run this model with precision f32m or f64)' if precision == 'f16' else ''))
        names = np.empty(sk.n_out, dtype=object)
        names[:] = sk.names_bytes()
        res = [poses, sk.edges_array(), names]
        if return_uncertainty:
            from metro_pose3d_amd.heads import place_covariances
            res.append(PoseUncertainty(*place_covariances(cov01, peak, eng.spec)) if n else
                       PoseUncertainty(poses.new_empty((0, sk.n_out, 3, 3)), poses.new_empty((0, sk.n_out))))
        if return_heatmaps:
            res.append(Heatmaps(heat_xy, heat_z))
        po = torch.cat(posts) if posts else f32(0, sk.n_out, Engine.POST_STATS)
        res.append(posterior_to_metric(eng.spec, po, coords01))
    return tuple(res)


def visualize_pose(image, coords, edges):
    """Stick-figure plot like reference inference.py:46-76 (matplotlib optional)."""
    import matplotlib
    matplotlib.use(os.environ.get('MPLBACKEND', 'Agg'))
    import matplotlib.pyplot as plt
    from mpl_toolkits.mplot3d import Axes3D  # noqa: F401

    pts = np.asarray(coords, dtype=np.float64)
    # camera frame has y down / z forward; matplotlib wants z up (reference inference.py:52-56)
    plot_pts = np.stack([pts[:, 0], pts[:, 2], -pts[:, 1]], axis=1)
    fig = plt.figure(figsize=(10, 5))
    ax_im = fig.add_subplot(1, 2, 1)
    ax_im.set_title('Input')
    ax_im.imshow(np.clip(np.asarray(image), 0, 1))
    ax = fig.add_subplot(1, 2, 2, projection='3d')
    ax.set_title('Prediction')
    lim = 800
    ax.set_xlim3d(-lim, lim); ax.set_ylim3d(-lim, lim); ax.set_zlim3d(-lim, lim)
    for a, b in np.asarray(edges):
        ax.plot(*zip(plot_pts[a], plot_pts[b]), marker='o', markersize=2)
    ax.scatter(plot_pts[:, 0], plot_pts[:, 1], plot_pts[:, 2], s=2)
    fig.tight_layout()
    return fig


def main(argv=None):
    parser = argparse.ArgumentParser(description='MeTRo-Pose3D on MI355X', allow_abbrev=False)
    parser.add_argument('--model-path', type=str, required=True)
    parser.add_argument('--image', type=str, default=None,
                        help='.npy file with a [256,256,3] float image in [0,1]; default: seeded noise')
    parser.add_argument('--precision', type=str, default=None, choices=['f16', 'f32', 'f32m', 'f64'])
    parser.add_argument('--plot', type=str, default=None, help='write the stick-figure plot to this file')
    parser.add_argument('--frame', type=str, default=None,
                        help='.npy file with a uint8 [H,W,3] RGB frame (or --pixel-format): poses of the --box persons in it '
                             '(frames.py)')
    parser.add_argument('--box', type=str, action='append', default=[], help='x,y,w,h of a person box in --frame (repeatable)')
    parser.add_argument('--intrinsics', type=str, default=None, help='fx,fy,cx,cy of the --frame camera')
    parser.add_argument('--distortion', type=str, default=None, help='k1,k2,p1,p2,k3 of the --frame camera (needs --intrinsics)')
    parser.add_argument('--bone-lengths', type=str, default=None,
                        help='.npy with the bone lengths in mm over the model\'s head edges ([E] or [boxes, E]): absolute '
                             'camera-frame poses and frame pixels of the --box persons (needs --intrinsics)')
    parser.add_argument('--root-depth', type=str, default=None,
                        help='MM[,MM...]: root depth of every --box person in its crop\'s virtual camera (true-root-depth '
                             'scale recovery; needs --intrinsics)')
    parser.add_argument('--views', type=int, default=None,
                        help='N: test-time augmentation, N rolled / flipped views per --box averaged (the default view set of '
                             'frames.view_set: rolls -20..+20 degrees, flips on odd views; 1 to 32)')
    parser.add_argument('--pixel-format', type=str, default=None, choices=['rgb', 'bgr', 'nv12', 'i420'],
                        help='layout of --frame: rgb / bgr uint8 [H,W,3] (default rgb), nv12 / i420 uint8 [H*3/2,W] (Y rows, '
                             'then the chroma rows as ffmpeg -f rawvideo writes them); converted per tap in the warp')
    parser.add_argument('--color-matrix', type=str, default=None, choices=['bt601', 'bt709'],
                        help='YUV matrix of an nv12 / i420 --frame (limited range; default bt601, OpenCV\'s)')
    parser.add_argument('--crop-dtype', type=str, default=None, choices=['float32', 'uint8'],
                        help="dtype of the crops the warp cuts from --frame: 'float32' (default) or 'uint8' (the remapped bytes, "
                             'read by the network as they are: the same poses from a quarter of the crop bytes)')
    parser.add_argument('--uncertainty', action='store_true',
                        help='also print, per joint, the standard deviations in mm of its heat-map along the three axes and its '
                             'peak probability')
    parser.add_argument('--heatmaps', type=str, default=None, metavar='OUT.npz',
                        help='also write every joint\'s heat-map marginals of the crop call to this .npz: xy [1,J,S,S] and '
                             'z [1,J,D] (output joint order), next to the poses and the joint names')
    parser.add_argument('--modes', type=str, default=None, metavar='K[,R]',
                        help='also print, per joint, its heat-map modes that hold a mass of at least 0.05: up to K places the '
                             'joint may be (window radius R voxels, default 1), each with its mass and position in mm')
    parser.add_argument('--skeleton', type=str, default=None, metavar='BONES.npy',
                        help='with --modes: choose among every joint\'s modes by these bone lengths ([E] mm over the skeleton\'s '
                             'edges, NaN: unknown); prints the joints whose choice is not mode 0, their marginals and the evidence')
    parser.add_argument('--prior', type=str, default=None, metavar='PRIOR.npz',
                        help='also print, per joint, its heat-map posterior under the Gaussian prior of this .npz (arrays '
                             '`positions` [Jout,3] mm, crop-metric frame, and `precision` [Jout,3,3] 1/mm^2): the posterior '
                             'position, its standard deviations and exp(log_evidence)')
    opts = parser.parse_args(argv)
    modes_kr = None
    if opts.modes:
        try:
            modes_kr = [int(v) for v in opts.modes.split(',')]
            modes_kr = (modes_kr[0], modes_kr[1] if len(modes_kr) > 1 else 1)
            if len(opts.modes.split(',')) > 2:
                raise ValueError(opts.modes)
        except (ValueError, IndexError):
            parser.error(f'--modes takes K or K,R (integers), got {opts.modes!r}')
    if opts.frame:
        if opts.heatmaps or opts.modes or opts.prior or opts.skeleton:
            parser.error('--heatmaps, --modes, --skeleton and --prior go with the crop call (--image), not with --frame')
        return _main_frame(opts)
    if opts.crop_dtype:
        parser.error('--crop-dtype goes with --frame')
    if opts.box or opts.intrinsics or opts.distortion or opts.bone_lengths or opts.root_depth or opts.views is not None:
        parser.error('--box, --intrinsics, --distortion, --bone-lengths, --root-depth and --views go with --frame')
    if opts.pixel_format or opts.color_matrix:
        parser.error('--pixel-format and --color-matrix go with --frame')
    if opts.image:
        img = np.load(opts.image).astype(np.float32)
    else:
        from metro_pose3d_amd.synth import make_images
        img = make_images(1)[0]
    images = torch.from_numpy(img[None])
    modes = posterior = chosen = None
    if opts.skeleton and not modes_kr:
        parser.error('--skeleton chooses among modes: it needs --modes K[,R]')
    if opts.prior:
        if modes_kr:
            parser.error('--prior and --modes are two calls: give one of them')
        with np.load(opts.prior) as f:
            prior_pos, prior_lam = np.asarray(f['positions'], np.float64), np.asarray(f['precision'], np.float64)
        prior_pos = prior_pos[None] if prior_pos.ndim == 2 else prior_pos
        prior_lam = prior_lam[None] if prior_lam.ndim == 3 else prior_lam
        poses, edges, names, *more, posterior = estimate_pose_posterior(images, opts.model_path, prior_pos, prior_lam, precision=opts.precision,
                                                                        return_uncertainty=opts.uncertainty, return_heatmaps=bool(opts.heatmaps))
    elif modes_kr and opts.skeleton:
        try:
            poses, edges, names, *more, modes, chosen = estimate_pose_skeleton(
                images, opts.model_path, np.load(opts.skeleton), modes_kr[0], modes_kr[1], precision=opts.precision,
                return_uncertainty=opts.uncertainty, return_heatmaps=bool(opts.heatmaps))
        except ValueError as e:
            raise SystemExit(str(e))
    elif modes_kr:
        poses, edges, names, *more, modes = estimate_pose_modes(images, opts.model_path, modes_kr[0], modes_kr[1], precision=opts.precision,
                                                                return_uncertainty=opts.uncertainty, return_heatmaps=bool(opts.heatmaps))
    else:
        poses, edges, names, *more = estimate_pose(images, opts.model_path, precision=opts.precision,
                                                   return_uncertainty=opts.uncertainty, return_heatmaps=bool(opts.heatmaps))
    unc = more[:1] if opts.uncertainty else []
    poses = poses.cpu().numpy()
    if opts.heatmaps:
        np.savez(opts.heatmaps, xy=more[-1].xy.cpu().numpy(), z=more[-1].z.cpu().numpy(), poses=poses,
                 joint_names=np.array([nm.decode() for nm in names]))
    tails = _uncertainty_columns(unc[0], 0) if unc else [''] * len(names)
    for name, p, tail in zip(names, poses[0], tails):
        print(f'{name.decode():>10s}  {p[0]:9.2f} {p[1]:9.2f} {p[2]:9.2f}{tail}')
    if modes is not None:
        mass, at = modes.mass[0].cpu().numpy(), modes.poses[0].cpu().numpy()
        for r, name in enumerate(names):
            for i in np.flatnonzero(mass[r] >= 0.05):
                print(f'{name.decode():>10s}  mode {i}: mass {mass[r, i]:.3f} at {at[r, i, 0]:9.2f} {at[r, i, 1]:9.2f} {at[r, i, 2]:9.2f}')
    if chosen is not None:
        choice, prob = chosen.choice[0].cpu().numpy(), chosen.prob[0].cpu().numpy()
        ev, at = chosen.log_evidence[0].cpu().numpy(), chosen.poses[0].cpu().numpy()
        moved = np.flatnonzero(choice > 0)
        print(f'skeleton: {len(moved)} of {len(names)} joints are not in their first mode')
        for r in moved:
            marginals = ' '.join(f'{v:.3f}' for v in prob[r])
            print(f'{names[r].decode():>10s}  mode {choice[r]}: marginals {marginals}   log evidence {ev[r]:8.3f}   selected pose '
                  f'{at[r, 0]:9.2f} {at[r, 1]:9.2f} {at[r, 2]:9.2f}')
    if posterior is not None:
        at, ev = posterior.positions[0].cpu().numpy(), np.exp(posterior.log_evidence[0].double().cpu().numpy())
        sd = np.sqrt(np.maximum(np.diagonal(posterior.covariance[0].cpu().numpy(), axis1=-2, axis2=-1), 0.0))
        for r, name in enumerate(names):
            print(f'{name.decode():>10s}  posterior at {at[r, 0]:9.2f} {at[r, 1]:9.2f} {at[r, 2]:9.2f}   sd {sd[r, 0]:7.2f} {sd[r, 1]:7.2f} '
                  f'{sd[r, 2]:7.2f} mm   evidence {ev[r]:6.4f}')
    if opts.plot:
        visualize_pose(img, poses[0], edges).savefig(opts.plot)


def _uncertainty_columns(unc, k):
    """Per joint of pose k: '   sd x y z mm   peak p' from a PoseUncertainty-like (covariance, peak)."""
    cov, peak = unc[0][k].cpu().numpy(), unc[1][k].cpu().numpy()
    sd = np.sqrt(np.maximum(np.diagonal(cov, axis1=-2, axis2=-1), 0.0))
    return [f'   sd {s[0]:7.2f} {s[1]:7.2f} {s[2]:7.2f} mm   peak {p:6.4f}' for s, p in zip(sd, peak)]


def _floats(text, n, flag):
    v = [float(t) for t in text.split(',')]
    if len(v) != n:
        raise SystemExit(f'{flag} takes {n} comma-separated numbers, got {text!r}')
    return v


def _main_frame(opts):
    from metro_pose3d_amd.frames import Camera, estimate_pose_in_frames
    frame = np.load(opts.frame)
    if not opts.box:
        raise SystemExit('--frame needs at least one --box x,y,w,h')
    boxes = np.array([_floats(b, 4, '--box') for b in opts.box])
    camera = None
    if opts.intrinsics:
        fx, fy, cx, cy = _floats(opts.intrinsics, 4, '--intrinsics')
        dist = _floats(opts.distortion, 5, '--distortion') if opts.distortion else None
        camera = Camera(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]]), dist)
    elif opts.distortion:
        raise SystemExit('--distortion needs --intrinsics')
    fmt = dict(pixel_format=opts.pixel_format or 'rgb', color_matrix=opts.color_matrix or 'bt601',
               crop_dtype=opts.crop_dtype or 'float32')
    if opts.bone_lengths or opts.root_depth:
        return _main_locate(opts, frame, boxes, camera, fmt)
    try:
        poses, edges, names, *unc = estimate_pose_in_frames(frame, boxes, opts.model_path, cameras=camera,
                                                            precision=opts.precision, views=opts.views,
                                                            return_uncertainty=opts.uncertainty, **fmt)
    except ValueError as e:
        raise SystemExit(str(e))
    for k, pose in enumerate(poses.cpu().numpy()):
        print(f'box {k} {opts.box[k]} (camera frame, root-relative mm)')
        tails = _uncertainty_columns(unc[0], k) if unc else [''] * len(names)
        for name, p, tail in zip(names, pose, tails):
            print(f'{name.decode():>10s}  {p[0]:9.2f} {p[1]:9.2f} {p[2]:9.2f}{tail}')


def _main_locate(opts, frame, boxes, camera, fmt):
    from metro_pose3d_amd.frames import locate_poses_in_frames
    if opts.bone_lengths and opts.root_depth:
        raise SystemExit('--bone-lengths and --root-depth are two scale recoveries: pick one')
    if camera is None:
        raise SystemExit('--bone-lengths / --root-depth place the poses metrically: they need --intrinsics')
    if opts.bone_lengths:
        kw = dict(scale_recovery='bone-lengths', bone_lengths=np.load(opts.bone_lengths))
    else:
        kw = dict(scale_recovery='true-root-depth', root_depth=_floats(opts.root_depth, len(boxes), '--root-depth'))
    try:
        res = locate_poses_in_frames(frame, boxes, opts.model_path, cameras=camera, precision=opts.precision, views=opts.views,
                                     return_uncertainty=opts.uncertainty, **kw, **fmt)
    except ValueError as e:
        raise SystemExit(str(e))
    poses, kp, z = res.poses.cpu().numpy(), res.keypoints2d.cpu().numpy(), res.z_offset.cpu().numpy()
    for k in range(len(boxes)):
        print(f'box {k} {opts.box[k]} (camera frame, absolute mm; frame pixels); root depth {z[k]:.1f} mm')
        tails = _uncertainty_columns((res.covariance, res.peak), k) if opts.uncertainty else [''] * len(res.joint_names)
        for name, p, q, tail in zip(res.joint_names, poses[k], kp[k], tails):
            print(f'{name.decode():>10s}  {p[0]:9.2f} {p[1]:9.2f} {p[2]:9.2f}   px {q[0]:8.2f} {q[1]:8.2f}{tail}')


if __name__ == '__main__':
    main()
