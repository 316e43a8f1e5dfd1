#!/usr/bin/env python3
"""Frames in other pixel formats: what converting in the warp (metro_warp_crops_frames_planes) costs and saves.

    python tools/yuv_frames_probe.py [--out FILE] [--quick]          # one JSON object on stdout (and in FILE)

Inputs of tools/device_geometry_probe.py: 64 boxes from 8 frames of 1920 x 1080, RN50 stride 16 h36m (synthetic weights), f16.
  * us per warp launch (64 crops of 256^2) for 'rgb' (metro_warp_crops_frames_u8), 'bgr', 'nv12' and 'i420' device frames, in
    the homography mode (an undistorted camera) and the distorted mode (H36M-like coefficients): device events around 200
    back-to-back launches after 20 warm-up launches, median of 5 windows;
  * crops/s of estimate_pose_in_frames with device geometry (CUDA boxes, distorted camera) from HOST nv12 frames against host
    rgb frames (the upload: 1.5 against 3 bytes per pixel);
  * crops/s from DEVICE nv12 frames against what a caller does without the feature: convert NV12 -> RGB with torch ops on the
    device (the same integer rule), then the 'rgb' call;
host clock around calls that end in the call's own synchronisation, after 3 warm-up calls, median of 5 windows of 10 calls.
For the kernel rows of the profiler: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/yuv_frames_probe.py --quick
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from metro_pose3d_amd import ModelSpec, save_model, synth  # noqa: E402
from metro_pose3d_amd import frames as FR  # noqa: E402
from metro_pose3d_amd.frames import Camera, estimate_pose_in_frames  # noqa: E402
from tools.device_geometry_probe import launch_us, per_s  # noqa: E402

BT601 = (1220542, 1673527, -852492, -409993, 2116026)


def torch_nv12_to_rgb(f: torch.Tensor) -> torch.Tensor:
    """uint8 [H*3/2, W] NV12 on the device -> uint8 [H, W, 3] RGB with torch ops: OpenCV's integer BT.601 rule, the
    conversion a caller would write without pixel_format='nv12'."""
    cy, cvr, cvg, cug, cub = BT601
    h = f.shape[0] * 2 // 3
    y = (f[:h].to(torch.int32) - 16).clamp_(min=0) * cy + (1 << 19)
    uv = f[h:].view(h // 2, -1, 2).to(torch.int32) - 128
    uv = uv.repeat_interleave(2, 0).repeat_interleave(2, 1)
    u, v = uv[..., 0], uv[..., 1]
    rgb = torch.stack([y + cvr * v, y + cvg * v + cug * u, y + cub * u], -1) >> 20
    return rgb.clamp_(0, 255).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the JSON object to this file')
    ap.add_argument('--quick', action='store_true', help='fewer windows (under a profiler)')
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('yuv_frames_probe: no HIP device (these numbers exist only on the GPU)')
    windows, iters, calls = (2, 20, 2) if opts.quick else (5, 200, 10)
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    h, w = 1080, 1920
    nv12_host = [rng.integers(0, 256, (h * 3 // 2, w), dtype=np.uint8) for _ in range(8)]
    nv12 = [torch.from_numpy(f).to(dev) for f in nv12_host]
    rgb = [torch_nv12_to_rgb(f) for f in nv12]
    rgb_host = [f.cpu().numpy() for f in rgb]
    i420 = [torch.cat([f[:h].reshape(-1), f[h:].view(-1, 2)[:, 0], f[h:].view(-1, 2)[:, 1]]).view(h * 3 // 2, w) for f in nv12]
    bgr = [f.flip(-1).contiguous() for f in rgb]
    # the YUV -> RGB rule of the kernel and of torch_nv12_to_rgb agree: checked once, on the crops, below
    k = np.array([[1500., 0, 960], [0, 1500, 540], [0, 0, 1]])
    dist = np.float32([-0.2071, 0.2479, -0.00142, -0.00098, -0.00309])
    fi = np.repeat(np.arange(8), 8)
    n = len(fi)
    boxes = np.array([[rng.uniform(100, 1500), rng.uniform(50, 500), rng.uniform(150, 300), rng.uniform(300, 500)] for _ in fi])
    d_boxes, d_fi = torch.from_numpy(boxes).to(dev), torch.from_numpy(fi).to(dev)
    spec = ModelSpec(50, 16, 'h36m')
    side = spec.proc_side
    result = {'device': torch.cuda.get_device_name(dev),
              'calls': '64 crops of 256^2 from 8 frames of 1920x1080, RN50 stride 16 h36m (synthetic weights), f16; warp '
                       'launches from device frames; estimate_pose_in_frames with device geometry (CUDA boxes), distorted '
                       'camera'}
    out = torch.empty((n, side, side, 3), dtype=torch.float32, device=dev)
    sets = {'rgb': FR._device_frames(rgb, dev), 'bgr': FR._device_frames(FR._frame_set(bgr, 'bgr'), dev),
            'nv12': FR._device_frames(FR._frame_set(nv12, 'nv12'), dev),
            'i420': FR._device_frames(FR._frame_set(i420, 'i420'), dev)}
    for mode, cam in (('homography', Camera(k)), ('distorted', Camera(k, dist))):
        crops = FR._upload(FR.pack_crops(FR.crop_params(cam, boxes, fi, side), fi), dev)
        ref = None
        for fmt, devf in sets.items():
            launch = lambda: FR._launch_warp(devf, crops, n, side, out, dev)
            result[f'warp_us_64_{fmt}_{mode}'] = launch_us(launch, windows, iters)
            if ref is None:
                ref = out.clone()
            elif not torch.equal(out, ref):
                raise SystemExit(f'yuv_frames_probe: {fmt} crops differ from the rgb crops ({mode})')
        for fmt in ('bgr', 'nv12', 'i420'):
            result[f'warp_ratio_{fmt}_to_rgb_{mode}'] = round(result[f'warp_us_64_{fmt}_{mode}']['median'] /
                                                              result[f'warp_us_64_rgb_{mode}']['median'], 3)
    cam = Camera(k, dist)
    params = synth.make_params(spec.arch, spec.n_head_channels, spec.base_width, seed=0,
                               logit_gain=synth.logit_gain_for(50, 16))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'rn50_s16.npz')
        save_model(path, spec, params)
        kw = dict(cameras=cam, frame_index=d_fi, precision='f16')
        runs = {
            'host_rgb': lambda: estimate_pose_in_frames(rgb_host, d_boxes, path, **kw),
            'host_nv12': lambda: estimate_pose_in_frames(nv12_host, d_boxes, path, pixel_format='nv12', **kw),
            'device_nv12': lambda: estimate_pose_in_frames(nv12, d_boxes, path, pixel_format='nv12', **kw),
            'device_nv12_torch_convert_then_rgb': lambda: estimate_pose_in_frames([torch_nv12_to_rgb(f) for f in nv12],
                                                                                  d_boxes, path, **kw),
        }
        a, b = runs['device_nv12'](), runs['device_nv12_torch_convert_then_rgb']()
        if not torch.equal(a[0], b[0]):
            raise SystemExit('yuv_frames_probe: nv12 poses differ from the torch-converted rgb poses')
        for name, fn in runs.items():
            result[f'crops_per_s_estimate_pose_in_frames_{name}'] = per_s(fn, n, windows, calls)
    c = {k2: v['median'] for k2, v in result.items() if k2.startswith('crops_per_s')}
    result['speedup_host_nv12_over_host_rgb'] = round(c['crops_per_s_estimate_pose_in_frames_host_nv12'] /
                                                      c['crops_per_s_estimate_pose_in_frames_host_rgb'], 2)
    result['speedup_device_nv12_over_torch_convert'] = round(
        c['crops_per_s_estimate_pose_in_frames_device_nv12'] /
        c['crops_per_s_estimate_pose_in_frames_device_nv12_torch_convert_then_rgb'], 2)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, 'w') as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
