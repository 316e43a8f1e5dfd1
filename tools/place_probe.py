#!/usr/bin/env python3
"""Absolute poses and frame keypoints: what metro_place_poses and locate_poses_in_frames cost on the GPU.

    python tools/place_probe.py [--out FILE]          # one JSON object on stdout (and in FILE)

  * us per metro_place_poses launch at n = 64 and 256 crops, scale recovery bone-lengths (the per-crop Levenberg-Marquardt
    solve dominates), camera coords, keypoints on, H36M-like distorted camera: device events around 200 back-to-back launches
    of the C entry (inputs uploaded once) after 20 warm-up launches, median of 5 windows;
  * calls/s of locate_poses_in_frames (bone-lengths, camera coords) against estimate_pose_in_frames (camera coords) on the
    same 64 boxes from 8 uint8 host frames of 1920 x 1080, RN50 stride 16 h36m (synthetic weights), f16: host clock around
    calls that end in the call's own synchronisation, after 3 warm-up calls, median of 5 windows of 10 calls.  Both calls
    are bounded by the host geometry (look_at_box per box).
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
from metro_pose3d_amd.frames import (Camera, estimate_pose_in_frames, locate_poses_in_frames, pack_placements,  # noqa: E402
                                     placement_params)


def launch_us(spec, n, cam, rng, windows, iters):
    dev = torch.device('cuda', 0)
    sk = spec.skeleton
    boxes = np.array([[rng.uniform(100, 1500), rng.uniform(50, 500), rng.uniform(150, 300), rng.uniform(300, 500)]
                      for _ in range(n)])
    q = placement_params(cam, boxes, np.zeros(n, np.int64), spec.proc_side)
    c01 = torch.from_numpy(rng.uniform(0.3, 0.7, (n, sk.n_head, 3)).astype(np.float32)).to(dev)
    recs = torch.from_numpy(pack_placements(q)).to(dev)
    bones = torch.from_numpy(rng.uniform(200, 450, len(sk.head_edges))).to(dev)
    edges = torch.from_numpy(np.asarray(sk.head_edges, np.int32)).to(dev)
    mirror = torch.from_numpy(np.asarray(sk.out_mirror, np.int32)).to(dev)
    out = torch.empty((n, sk.n_out, 3), device=dev)
    kp = torch.empty((n, sk.n_out, 2), device=dev)
    z = torch.empty(n, device=dev)
    cs = spec.to_c(0)
    lib, stream = _lib.load(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    launch = lambda: _lib.check(lib.metro_place_poses(p(c01), None, p(recs), n, C.byref(cs), _lib.METRO_SCALE_BONE_LENGTHS,
                                                      p(bones), 0, None, p(edges), len(sk.head_edges), p(mirror),
                                                      _lib.METRO_COORDS_CAMERA, p(out), p(kp), p(z), stream), 'metro_place_poses')
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


def calls_per_s(fn, windows, calls):
    for _ in range(3):
        fn()
    res = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        res.append(calls / (time.perf_counter() - t0))
    return statistics.median(res), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the JSON object to this file')
    ap.add_argument('--quick', action='store_true', help='fewer windows (under a profiler)')
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('place_probe: no HIP device (these numbers exist only on the GPU)')
    windows, iters, calls = (2, 20, 2) if opts.quick else (5, 200, 10)
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    k = np.array([[1500., 0, 960], [0, 1500, 540], [0, 0, 1]])
    cam = Camera(k, np.float32([-0.2071, 0.2479, -0.00142, -0.00098, -0.00309]))
    spec = ModelSpec(50, 16, 'h36m')
    result = {'device': torch.cuda.get_device_name(dev),
              'launch': 'metro_place_poses, bone-lengths, camera coords, keypoints, distorted camera, h36m (17 joints, 16 edges)'}
    for n in (64, 256):
        med, all_ = launch_us(spec, n, cam, rng, windows, iters)
        result[f'place_us_n{n}'] = {'median': round(med, 2), 'windows': [round(v, 2) for v in all_]}
    host = [rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8) for _ in range(8)]
    fi = np.repeat(np.arange(8), 8)
    boxes = np.array([[rng.uniform(100, 1500), rng.uniform(50, 500), rng.uniform(150, 300), rng.uniform(300, 500)] for _ in fi])
    bones = rng.uniform(200, 450, len(spec.skeleton.head_edges))
    params = synth.make_params(spec.arch, spec.n_head_channels, spec.base_width, seed=0,
                               logit_gain=synth.logit_gain_for(50, 16))
    result['calls'] = '64 boxes from 8 uint8 host frames of 1920x1080, RN50 stride 16 h36m (synthetic weights), f16'
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'rn50_s16.npz')
        save_model(path, spec, params)
        for name, fn in (('estimate_pose_in_frames',
                          lambda: estimate_pose_in_frames(host, boxes, path, cameras=cam, frame_index=fi, precision='f16')),
                         ('locate_poses_in_frames',
                          lambda: locate_poses_in_frames(host, boxes, path, cameras=cam, frame_index=fi, bone_lengths=bones,
                                                         precision='f16'))):
            med, all_ = calls_per_s(fn, windows, calls)
            result[f'calls_per_s_{name}'] = {'median': round(med, 2), 'windows': [round(v, 2) for v in all_]}
    result['locate_over_estimate'] = round(result['calls_per_s_locate_poses_in_frames']['median'] /
                                           result['calls_per_s_estimate_pose_in_frames']['median'], 3)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, 'w') as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
