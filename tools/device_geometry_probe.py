#!/usr/bin/env python3
"""Crop geometry on the device against the host: what `geometry=` changes for the full-frame calls.

    python tools/device_geometry_probe.py [--out FILE] [--quick]          # one JSON object on stdout (and in FILE)

Same inputs as tools/frames_probe.py: 64 boxes from 8 uint8 device frames of 1920 x 1080, RN50 stride 16 h36m (synthetic
weights), f16, an undistorted and a distorted (H36M-like coefficients) camera.  For each camera, host geometry (host boxes,
per-box NumPy look_at_box) against device geometry (the same boxes as a CUDA tensor, one metro_look_at_boxes launch):
  * crops/s of estimate_pose_in_frames;
  * calls/s of locate_poses_in_frames (bone-lengths, camera coords) at views=None and views=5;
host clock around calls that end in the call's own synchronisation, after 3 warm-up calls, median of 5 windows of 10 calls;
  * us per metro_look_at_boxes launch at 64 boxes (the C entry alone, camera table uploaded once): device events around 200
    back-to-back launches after 20 warm-up launches, median of 5 windows.
For the kernel rows of the profiler: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/device_geometry_probe.py --quick
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
from metro_pose3d_amd import frames as FR  # noqa: E402
from metro_pose3d_amd.frames import Camera, estimate_pose_in_frames, locate_poses_in_frames  # noqa: E402


def launch_us(launch, windows, iters):
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
    return {'median': round(statistics.median(res), 2), 'windows': [round(v, 2) for v in res]}


def per_s(fn, units, windows, calls):
    for _ in range(3):
        fn()
    res = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        res.append(units * calls / (time.perf_counter() - t0))
    return {'median': round(statistics.median(res), 1), 'windows': [round(v, 1) for v in res]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the JSON object to this file')
    ap.add_argument('--quick', action='store_true', help='fewer windows (under a profiler)')
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('device_geometry_probe: no HIP device (these numbers exist only on the GPU)')
    windows, iters, calls = (2, 20, 2) if opts.quick else (5, 200, 10)
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    host = [rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8) for _ in range(8)]
    frames = [torch.from_numpy(f).to(dev) for f in host]
    k = np.array([[1500., 0, 960], [0, 1500, 540], [0, 0, 1]])
    dist = np.float32([-0.2071, 0.2479, -0.00142, -0.00098, -0.00309])
    fi = np.repeat(np.arange(8), 8)
    n = len(fi)
    boxes = np.array([[rng.uniform(100, 1500), rng.uniform(50, 500), rng.uniform(150, 300), rng.uniform(300, 500)] for _ in fi])
    d_boxes, d_fi = torch.from_numpy(boxes).to(dev), torch.from_numpy(fi).to(dev)
    spec = ModelSpec(50, 16, 'h36m')
    bones = rng.uniform(200, 450, len(spec.skeleton.head_edges))
    result = {'device': torch.cuda.get_device_name(dev),
              'calls': '64 boxes from 8 uint8 device frames of 1920x1080, RN50 stride 16 h36m (synthetic weights), f16; '
                       'host geometry: host boxes; device geometry: the same boxes as a CUDA float64 tensor, CUDA frame_index; '
                       'locate: bone-lengths, camera coords; views=5 is the default set'}
    lib, stream = _lib.load(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    d_fi32 = d_fi.to(torch.int32)
    bases = torch.empty((n, FR.VIEW_BASE_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    p = lambda x: C.c_void_p(x.data_ptr())
    cameras = {'undistorted': Camera(k), 'distorted': Camera(k, dist)}
    for name, cam in cameras.items():
        table = torch.from_numpy(FR.pack_frame_cameras(cam, 8).view(np.uint8)).to(dev)
        launch = lambda: _lib.check(lib.metro_look_at_boxes(p(d_boxes), p(d_fi32), n, 8, p(table), 1, spec.proc_side,
                                                            p(bases), p(status), stream), 'metro_look_at_boxes')
        result[f'look_at_boxes_us_64_{name}'] = launch_us(launch, windows, iters)
    params = synth.make_params(spec.arch, spec.n_head_channels, spec.base_width, seed=0,
                               logit_gain=synth.logit_gain_for(50, 16))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'rn50_s16.npz')
        save_model(path, spec, params)
        for name, cam in cameras.items():
            for geo, b, f in (('host', boxes, fi), ('device', d_boxes, d_fi)):
                est = lambda: estimate_pose_in_frames(frames, b, path, cameras=cam, frame_index=f, precision='f16')
                result[f'crops_per_s_estimate_pose_in_frames_{name}_{geo}'] = per_s(est, n, windows, calls)
                for views in (None, 5):
                    loc = lambda: locate_poses_in_frames(frames, b, path, cameras=cam, frame_index=f, bone_lengths=bones,
                                                         precision='f16', views=views)
                    result[f'calls_per_s_locate_poses_in_frames_{name}_views_{views}_{geo}'] = per_s(loc, 1, windows, calls)
    for name in cameras:
        e_h = result[f'crops_per_s_estimate_pose_in_frames_{name}_host']['median']
        e_d = result[f'crops_per_s_estimate_pose_in_frames_{name}_device']['median']
        result[f'speedup_estimate_{name}'] = round(e_d / e_h, 2)
        for views in (None, 5):
            l_h = result[f'calls_per_s_locate_poses_in_frames_{name}_views_{views}_host']['median']
            l_d = result[f'calls_per_s_locate_poses_in_frames_{name}_views_{views}_device']['median']
            result[f'speedup_locate_{name}_views_{views}'] = round(l_d / l_h, 2)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, 'w') as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
