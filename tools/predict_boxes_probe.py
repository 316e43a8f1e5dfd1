#!/usr/bin/env python3
"""What predicting the next frames' person boxes from the track table costs: the two launches of metro_predict_boxes.

    python tools/predict_boxes_probe.py [--out FILE] [--quick]          # one JSON object on stdout (and in FILE)

J = 17; persons 0.5 m apart, 4 to 6.5 m in front of distorted 1920 x 1080 cameras, all live, so every (frame, slot) projects all
its joints and has a box.
  * us per metro_predict_boxes call (both launches: one thread per (frame, slot), then the one-workgroup compaction) at
    8 tracks x 1 frame without detections, and at 128 tracks x 64 frames with 1024 detections (half of them copies of predicted
    boxes, which are suppressed, half in empty places): device events around back-to-back calls of the C entry after 20 warm-up
    calls, median of 5 windows.  The table is read only, so nothing is reset between calls.
The expectation is a latency-bound call of a few us at the small shape; nothing here is a throughput figure.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from metro_pose3d_amd import _lib  # noqa: E402
from metro_pose3d_amd import frames as FR  # noqa: E402
from metro_pose3d_amd.camera import Camera  # noqa: E402

NJ, W, H = 17, 1920, 1080


def table_scene(rng, n_tracks):
    """-> (state [T, J, 28], ids [T]) of n_tracks persons, every joint with a state at t = 0."""
    cloud = rng.uniform(-1, 1, (n_tracks, NJ, 3)) * [250.0, 850.0, 100.0]
    centre = np.stack([500.0 * (np.arange(n_tracks) % 12) - 2750.0, np.zeros(n_tracks), 4000.0 + 250.0 * (np.arange(n_tracks) // 12)], 1)
    state = np.zeros((n_tracks, NJ, 28))
    state[..., :3] = centre[:, None] + cloud
    state[..., 3:6] = rng.uniform(-1000, 1000, (n_tracks, 1, 3))
    p = np.zeros((6, 6))
    p[:3, :3], p[3:, 3:] = 400.0 * np.eye(3), 9e4 * np.eye(3)
    state[..., 6:27] = p[np.triu_indices(6)]
    return state, np.arange(n_tracks, dtype=np.int32)


def windows_us(fn, windows, iters):
    for _ in range(20):
        fn()
    res = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        res.append(a.elapsed_time(b) * 1e3 / iters)
    return {'median': round(statistics.median(res), 2), 'windows': [round(v, 2) for v in res]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the JSON object to this file')
    ap.add_argument('--quick', action='store_true', help='fewer windows (under a profiler)')
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('predict_boxes_probe: no HIP device (these numbers exist only on the GPU)')
    windows, iters = (1, 10) if opts.quick else (5, 500)
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    result = {'device': torch.cuda.get_device_name(dev),
              'scene': f'J = {NJ}, every slot live and in view of distorted {W}x{H} cameras, coords camera, default keywords'}
    lib, stream = _lib.load(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    p = lambda x: C.c_void_p(x.data_ptr() if x is not None else 0)
    cam = Camera(np.array([[1500.0, 0, W / 2], [0, 1500.0, H / 2], [0, 0, 1]]), (-0.25, 0.08, 0.001, -0.0005, -0.01))
    cameras = up(FR.pack_frame_cameras(cam).view(np.uint8))
    for n_tracks, n_frames, m in ((8, 1, 0), (128, 64, 1024)):
        state, ids = (up(a) for a in table_scene(rng, n_tracks))
        sizes = np.ascontiguousarray(np.tile([W, H], (n_frames, 1)), np.int32)
        times = np.ascontiguousarray(0.03 + 0.001 * np.arange(n_frames))
        cap = n_frames * n_tracks + m
        i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
        dense, dense_joints = torch.empty((n_frames, n_tracks, 4), dtype=torch.float64, device=dev), i32(n_frames, n_tracks)
        outs = [torch.empty((cap, 4), dtype=torch.float64, device=dev), i32(cap), i32(cap), i32(cap), i32(cap), i32(cap), i32(5)]
        det = det_fi = None

        def launch():
            _lib.check(lib.metro_predict_boxes(p(state), p(ids), n_tracks, NJ, p(cameras), 1, C.c_void_p(sizes.ctypes.data),
                                               C.c_void_p(times.ctypes.data), n_frames, _lib.METRO_COORDS_CAMERA, 4e6, 1.0, 1.25, 2.0,
                                               300.0, 100.0, 8.0, 9, 1, p(det), p(det_fi), m if det is not None else 0, 0.3, p(dense),
                                               p(dense_joints), *[p(o) for o in outs], stream), 'metro_predict_boxes')
        if m:
            launch()                                            # the predicted boxes the detections are drawn from
            fi = rng.integers(0, n_frames, m).astype(np.int32)
            boxes = dense.cpu().numpy()[fi, rng.integers(0, n_tracks, m)]
            boxes[m // 2:] = [4.0, 4.0, 6.0, 6.0]               # a corner no person reaches
            det, det_fi = up(boxes), up(fi)
        key = f'predict_{n_tracks}x{n_frames}_m{m}'
        result[key + '_us'] = windows_us(launch, windows, iters)
        counts = outs[-1].tolist()
        result[key + '_counts'] = counts
        assert counts[1] == n_tracks * n_frames and counts[3] == 0 and counts[4] == 0 and counts[0] + counts[2] == cap, counts
    text = json.dumps(result, indent=1, sort_keys=True)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
