#!/usr/bin/env python3
"""Test-time views: what `views=` costs locate_poses_in_frames.

    python tools/views_probe.py [--out FILE] [--quick]          # one JSON object on stdout (and in FILE)

  * calls/s of locate_poses_in_frames (bone-lengths, camera coords) at views=None, 1 and 5 on 64 boxes from 8 uint8 host
    frames of 1920 x 1080 with a distorted camera, RN50 stride 16 h36m (synthetic weights), f16: host clock around calls that
    end in the call's own synchronisation, after 3 warm-up calls, median of 5 windows of 10 calls;
  * the host part of one call: pack_view_bases (every look_at_box and record of the call) for the 64 boxes, median of 20;
  * us per metro_expand_views (64 boxes x 5 views) and metro_merge_views (64 x 5 views, keypoints, z offsets, spread) launch:
    device events around 200 back-to-back launches of the C entry after 20 warm-up launches, median of 5 windows.
The kernel rows of a `rocprofv3 --kernel-trace --stats` run of this script are recorded next to its output.
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
from metro_pose3d_amd.frames import Camera, locate_poses_in_frames, view_set  # noqa: E402


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


def calls_per_s(fn, windows, calls):
    for _ in range(3):
        fn()
    res = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        res.append(calls / (time.perf_counter() - t0))
    return {'median': round(statistics.median(res), 2), 'windows': [round(v, 2) for v in res]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the JSON object to this file')
    ap.add_argument('--quick', action='store_true', help='fewer windows (under a profiler)')
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('views_probe: no HIP device (these numbers exist only on the GPU)')
    windows, iters, calls = (2, 20, 2) if opts.quick else (5, 200, 10)
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    k = np.array([[1500., 0, 960], [0, 1500, 540], [0, 0, 1]])
    cam = Camera(k, np.float32([-0.2071, 0.2479, -0.00142, -0.00098, -0.00309]))
    spec = ModelSpec(50, 16, 'h36m')
    sk = spec.skeleton
    host = [rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8) for _ in range(8)]
    fi = np.repeat(np.arange(8), 8)
    n = len(fi)
    boxes = np.array([[rng.uniform(100, 1500), rng.uniform(50, 500), rng.uniform(150, 300), rng.uniform(300, 500)] for _ in fi])
    bones = rng.uniform(200, 450, len(sk.head_edges))
    result = {'device': torch.cuda.get_device_name(dev),
              'calls': '64 boxes from 8 uint8 host frames of 1920x1080, distorted camera, RN50 stride 16 h36m (synthetic '
                       'weights), f16, bone-lengths, camera coords; views=5 is the default set (rolls -20..20 deg, flips on '
                       'views 1 and 3)'}

    t = []
    for _ in range(20):
        t0 = time.perf_counter()
        FR.pack_view_bases(cam, boxes, fi, spec.proc_side)
        t.append((time.perf_counter() - t0) * 1e3)
    result['host_pack_view_bases_ms_64_boxes'] = round(statistics.median(t), 3)

    vs = view_set(5)
    bases = FR.pack_view_bases(cam, boxes, fi, spec.proc_side)
    d_bases = torch.from_numpy(bases).to(dev)
    table = FR.view_table(vs)
    m = n * 5
    crops = torch.empty((m, C.sizeof(_lib.MetroCropWarp)), dtype=torch.uint8, device=dev)
    places = torch.empty((m, C.sizeof(_lib.MetroPlacement)), dtype=torch.uint8, device=dev)
    lib, stream = _lib.load(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda x: C.c_void_p(x.data_ptr())
    expand = lambda: _lib.check(lib.metro_expand_views(p(d_bases), n, table, 5, spec.proc_side, p(crops), p(places), stream),
                                'metro_expand_views')
    result['expand_views_us_64x5'] = launch_us(expand, windows, iters)
    poses = torch.from_numpy(rng.normal(0, 300, (m, sk.n_out, 3)).astype(np.float32)).to(dev)
    kp = torch.from_numpy(rng.uniform(0, 1900, (m, sk.n_out, 2)).astype(np.float32)).to(dev)
    z = torch.from_numpy(rng.uniform(3000, 5000, m).astype(np.float32)).to(dev)
    mirror = torch.from_numpy(np.asarray(sk.out_mirror, np.int32)).to(dev)
    out, kout = torch.empty((n, sk.n_out, 3), device=dev), torch.empty((n, sk.n_out, 2), device=dev)
    zout, sout = torch.empty(n, device=dev), torch.empty((n, sk.n_out), device=dev)
    merge = lambda: _lib.check(lib.metro_merge_views(p(poses), p(kp), p(z), p(places), p(mirror), n, 5, sk.n_out, p(out), p(kout),
                                                     p(zout), p(sout), stream), 'metro_merge_views')
    result['merge_views_us_64x5'] = launch_us(merge, windows, iters)

    params = synth.make_params(spec.arch, spec.n_head_channels, spec.base_width, seed=0,
                               logit_gain=synth.logit_gain_for(50, 16))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'rn50_s16.npz')
        save_model(path, spec, params)
        for views in (None, 1, 5):
            fn = lambda: locate_poses_in_frames(host, boxes, path, cameras=cam, frame_index=fi, bone_lengths=bones,
                                                precision='f16', views=views)
            result[f'calls_per_s_views_{views}'] = calls_per_s(fn, windows, calls)
    r = lambda a, b: round(result[f'calls_per_s_views_{a}']['median'] / result[f'calls_per_s_views_{b}']['median'], 3)
    result['views_5_over_views_1'] = r(5, 1)
    result['views_1_over_views_None'] = r(1, None)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, 'w') as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
