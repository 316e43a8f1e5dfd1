#!/usr/bin/env python3
"""Frames in, poses out: what the new path costs on the GPU.

    python tools/frames_probe.py [--out FILE]          # one JSON object on stdout (and in FILE)

  * us per metro_warp_crops_frames_u8 launch, 64 crops of 256 x 256 from 8 uint8 frames of 1920 x 1080, in the homography
    mode (no distortion) and the general mode (H36M-like distortion): device events around 200 back-to-back launches of the
    C entry (crop records uploaded once) after 20 warm-up launches, median of 5 windows;
  * crops/s of estimate_pose_in_frames (host frames: upload + warp + forward + to_orig_cam) and of estimate_pose on the same
    64 crops already on the device, RN50 stride 16 h36m (synthetic weights), f16: host clock around calls that end in the
    call's own synchronisation, after 3 warm-up calls, median of 5 windows of 10 calls.
For kernel times from the profiler: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/frames_probe.py --quick
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from metro_pose3d_amd import ModelSpec, _lib, save_model, synth  # noqa: E402
from metro_pose3d_amd.frames import Camera, crop_params, estimate_pose_in_frames, pack_crops, warp_frames  # noqa: E402
from metro_pose3d_amd.inference import estimate_pose  # noqa: E402


def launch_us(frames, params, fi, windows, iters):
    """The C entry alone, records and frame table built once (warp_frames' host work would starve the device)."""
    dev = frames[0].device
    table = (_lib.MetroFrame * len(frames))()
    for k, f in enumerate(frames):
        table[k].data, table[k].h, table[k].w, table[k].row_stride = f.data_ptr(), f.shape[0], f.shape[1], f.stride(0)
    crops = torch.from_numpy(pack_crops(params, fi)).to(dev)
    out = torch.empty((len(fi), 256, 256, 3), dtype=torch.float32, device=dev)
    lib, stream = _lib.load(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    launch = lambda: _lib.check(lib.metro_warp_crops_frames_u8(table, len(frames), C.c_void_p(crops.data_ptr()), len(fi),
                                                               256, C.c_void_p(out.data_ptr()), stream))
    for _ in range(20):
        launch()
    res = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            launch()
        b.record()
        b.synchronize()
        res.append(a.elapsed_time(b) * 1e3 / iters)
    return statistics.median(res), res


def crops_per_s(fn, n, windows, calls):
    for _ in range(3):
        fn()
    res = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        res.append(n * calls / (time.perf_counter() - t0))
    return statistics.median(res), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the JSON object to this file')
    ap.add_argument('--quick', action='store_true', help='fewer windows (under a profiler)')
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('frames_probe: no HIP device (these numbers exist only on the GPU)')
    windows, iters, calls = (2, 20, 2) if opts.quick else (5, 200, 10)
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    host = [rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8) for _ in range(8)]
    frames = [torch.from_numpy(f).to(dev) for f in host]
    k = np.array([[1500., 0, 960], [0, 1500, 540], [0, 0, 1]])
    dist = np.float32([-0.2071, 0.2479, -0.00142, -0.00098, -0.00309])
    fi = np.repeat(np.arange(8), 8)
    boxes = np.array([[rng.uniform(100, 1500), rng.uniform(50, 500), rng.uniform(150, 300), rng.uniform(300, 500)] for _ in fi])
    result = {'shape': '64 crops of 256x256 from 8 uint8 frames of 1920x1080', 'device': torch.cuda.get_device_name(dev)}
    for mode, cam in (('homography', Camera(k)), ('general', Camera(k, dist))):
        p = crop_params(cam, boxes, fi, 256)
        med, all_ = launch_us(frames, p, fi, windows, iters)
        result[f'warp_us_{mode}'] = {'median': round(med, 2), 'windows': [round(v, 2) for v in all_]}
    t = []
    for _ in range(windows):
        t0 = time.perf_counter()
        crop_params(Camera(k, dist), boxes, fi, 256)
        t.append((time.perf_counter() - t0) * 1e3)
    result['host_ms_crop_params_64_boxes'] = {'median': round(statistics.median(t), 2), 'windows': [round(v, 2) for v in t]}
    spec = ModelSpec(50, 16, 'h36m')
    params = synth.make_params(spec.arch, spec.n_head_channels, spec.base_width, seed=0,
                               logit_gain=synth.logit_gain_for(50, 16))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'rn50_s16.npz')
        save_model(path, spec, params)
        cam = Camera(k, dist)
        crops = warp_frames(frames, crop_params(cam, boxes, fi, 256), fi, 256)
        for name, fn in (('estimate_pose_device_crops', lambda: estimate_pose(crops, path, precision='f16')),
                         ('estimate_pose_in_frames_host_frames',
                          lambda: estimate_pose_in_frames(host, boxes, path, cameras=cam, frame_index=fi, precision='f16')),
                         ('estimate_pose_in_frames_device_frames',
                          lambda: estimate_pose_in_frames(frames, boxes, path, cameras=cam, frame_index=fi, precision='f16'))):
            med, all_ = crops_per_s(fn, len(fi), windows, calls)
            result[f'crops_per_s_{name}'] = {'median': round(med, 1), 'windows': [round(v, 1) for v in all_]}
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, 'w') as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
