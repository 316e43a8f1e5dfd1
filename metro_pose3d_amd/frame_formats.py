"""Frames as decoders leave them, for the warp of the frame pipeline (frames.py): 'rgb' (the default), 'bgr' (OpenCV), 'nv12'
(hardware decoders), 'i420' (libavcodec's yuv420p).

  _frame_set, _planar     pixel_format / color_matrix and the layout of every frame, checked before any device work
  _device_frames          the frames on the device: packed uint8 [H, W, 3] tensors for metro_warp_crops_frames_u8 ('rgb'), or
                          plane views and descriptor fields for metro_warp_crops_frames_planes, which converts each tap as
                          the warp reads it (the others)

Divergence from the reference, on purpose:
  * a YUV frame ('nv12', 'i420') is the RGB image of OpenCV's integer cvtColor(COLOR_YUV2RGB_NV12 / _I420) rule (limited
    range, BT.601 by default or BT.709, the chroma of each 2x2 block replicated; include/metro_hip.h), not of ffmpeg's
    swscale, which rounds differently; a tap outside the frame is black (RGB 0), not YUV (0, 0, 0).
"""
from __future__ import annotations

from typing import NamedTuple, Tuple

import numpy as np
import torch

from metro_pose3d_amd import _lib

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


def _upload(a: np.ndarray, device: torch.device) -> torch.Tensor:
    """Host array -> device tensor without a host synchronisation (pinned staging, non-blocking copy)."""
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(device, non_blocking=True)


class _Planar(NamedTuple):
    """One frame for metro_warp_crops_frames_planes: its plane views (host or device) and the descriptor's fields."""
    planes: Tuple[torch.Tensor, ...]
    h: int
    w: int
    stride: Tuple[int, int]
    format: int
    matrix: int


class _FrameSet(NamedTuple):
    """Frames whose count and layouts are checked, as given (host or device data)."""
    items: list
    pixel_format: str
    color_matrix: str


def _frame_set(frames, pixel_format: str = 'rgb', color_matrix: str = 'bt601'):
    """Checks pixel_format and color_matrix and, for any format but 'rgb', the layout of every frame, before any device work.
    'rgb' frames come back as given (_device_frames checks them); the others as a _FrameSet.
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
    return _checked_frames(frames, pixel_format, color_matrix)


def _checked_frames(frames, pixel_format: str, color_matrix: str) -> _FrameSet:
    """One frame or many -> a _FrameSet of 1 to METRO_MAX_FRAMES frames whose layouts _planar accepts."""
    if pixel_format in ('rgb', 'bgr'):
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
    hwc = pixel_format in ('rgb', 'bgr')              # any strides: _device_frames packs the pixels

    def bad(what):
        return ValueError(f'frame {k}: {what}; pixel_format={pixel_format!r} takes {_LAYOUTS[pixel_format]}')

    def plane(t, name, ndim):
        t = torch.from_numpy(t) if isinstance(t, np.ndarray) else t
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != ndim:
            raise bad(f'{name} is {getattr(t, "dtype", type(t))} {tuple(getattr(t, "shape", ()))}')
        if not hwc and (t.stride(-1) != 1 or (ndim >= 2 and t.stride(0) < t.shape[1] * t.stride(1))):
            raise bad(f'{name} has strides {t.stride()}')
        return t

    def even(h, w):
        if h % 2 or w % 2:
            raise bad(f'{h} x {w} pixels (4:2:0 frames have an even height and width)')

    fmt, matrix = PIXEL_FORMATS[pixel_format], COLOR_MATRICES[color_matrix]
    if hwc:
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


def _device_frames(frames, device: torch.device):
    """The frames of a call on its device: host frames uploaded (pinned, non-blocking) at their own byte size, device frames
    as they are, an [H, W, 3] frame packed if it is not.  'rgb' frames (as given, checked here) -> uint8 [H, W, 3] tensors
    for metro_warp_crops_frames_u8; a _FrameSet of another format -> [_Planar] for metro_warp_crops_frames_planes."""
    fs = frames if isinstance(frames, _FrameSet) else _checked_frames(frames, 'rgb', 'bt601')
    hwc = fs.pixel_format in ('rgb', 'bgr')

    def to_device(k, a):
        if isinstance(a, tuple):
            return tuple(to_device(k, p) for p in a)
        t = torch.from_numpy(a) if isinstance(a, np.ndarray) else a
        if not t.is_cuda:
            return _upload(t.numpy(), device)
        if t.device != device:
            raise ValueError(f'frame {k} is on {t.device}, the call runs on {device}')
        if hwc and (t.stride(2) != 1 or t.stride(1) != 3 or t.stride(0) < 3 * t.shape[1]):
            t = t.contiguous()
        return t

    if fs.pixel_format == 'rgb':
        return [to_device(k, f) for k, f in enumerate(fs.items)]
    return [_planar(k, to_device(k, f), fs.pixel_format, fs.color_matrix) for k, f in enumerate(fs.items)]


def _first_frame(frames):
    """The first frame (or plane) of `frames`, from which a call without device boxes takes its device."""
    f = frames.items if isinstance(frames, _FrameSet) else frames
    while isinstance(f, (list, tuple)) and f:
        f = f[0]
    return f if isinstance(f, (torch.Tensor, np.ndarray)) else None
