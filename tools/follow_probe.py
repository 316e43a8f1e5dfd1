#!/usr/bin/env python3
"""What following persons over video costs: the metro_associate_tracks launch, and the whole call next to the tracking one.

    python tools/follow_probe.py [--out FILE] [--quick]          # one JSON object on stdout (and in FILE)

J = 17; persons on a 1 m grid drifting a few mm a frame, so every box continues its track and every step runs the whole walk
(costs, one greedy round per track, the filter step).
  * us per metro_associate_tracks launch at 8 tracks x 8 frames (64 boxes, capacity 64) and at 16 tracks x 64 frames (1024
    boxes, capacity 64), covariance measurements, from an empty table each time (the table is reset by three small device
    copies inside the timed window, which are timed on their own as `reset_us`): device events around back-to-back launches
    of the C entry after 20 warm-up launches, median of 5 windows;
  * calls/s of follow_poses_in_frames against track_poses_in_frames given the true track_index, on 8 tracks x 8 frames of
    1920 x 1080 uint8 frames with frames and boxes on the device, RN50 stride 32 h36m (synthetic weights), f16,
    true-root-depth.  Three arms INTERLEAVED window by window in one process: track, follow, track again.  The two track arms
    are the same code on the same data: their relative difference (`aa_spread`) is the noise margin the follow arm has to be
    read against.  Host clock around `calls` calls (each ends in its own synchronisation), after 3 warm-up windows, median of
    5 windows.
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
from metro_pose3d_amd.camera import Camera  # noqa: E402

FPS, NJ, CAPACITY = 32.0, 17, 64


def tracks_scene(rng, n_tracks, n_frames):
    """-> (poses [n, J, 3], cov [n, J, 9], times [n]) of n_tracks persons over n_frames frames, frame-major."""
    cloud = rng.uniform(-300, 300, (n_tracks, NJ, 3))
    v = rng.uniform(-8, 8, (n_tracks, 1, 3))
    centre = np.stack([1000.0 * (np.arange(n_tracks) % 4), 1000.0 * (np.arange(n_tracks) // 4), np.full(n_tracks, 3000.0)], 1)[:, None]
    poses = np.concatenate([centre + cloud + v * f + rng.normal(0, 2, cloud.shape) for f in range(n_frames)]).astype(np.float32)
    a = rng.normal(size=(len(poses), NJ, 3, 3))
    cov = (a @ a.transpose(0, 1, 3, 2) * 3 + 4 * np.eye(3)).astype(np.float32).reshape(len(poses), NJ, 9)
    return poses, cov, np.repeat(np.arange(n_frames) / FPS, n_tracks)


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


def interleaved_calls_per_s(arms, windows, calls):
    res = {k: [] for k, _ in arms}
    for w in range(3 + windows):
        for name, fn in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            if w >= 3:
                res[name].append(calls / (time.perf_counter() - t0))
    med = {k: statistics.median(v) for k, v in res.items()}
    a = 0.5 * (med['track'] + med['track_again'])
    out = {k: {'median': round(med[k], 2), 'windows': [round(v, 2) for v in res[k]]} for k in res}
    out['aa_spread'] = round(abs(med['track'] - med['track_again']) / a, 4)
    out['follow_over_track'] = round(med['follow'] / a, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the JSON object to this file')
    ap.add_argument('--quick', action='store_true', help='fewer windows (under a profiler)')
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('follow_probe: no HIP device (these numbers exist only on the GPU)')
    windows, iters, calls = (1, 10, 2) if opts.quick else (5, 100, 10)
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    result = {'device': torch.cuda.get_device_name(dev)}
    lib, stream = _lib.load(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    p = lambda x: C.c_void_p(x.data_ptr())
    cs = _lib.MetroSpec(n_joints_out=NJ)
    for n_tracks, n_frames in ((8, 8), (16, 64)):
        poses, cov, times = tracks_scene(rng, n_tracks, n_frames)
        n = len(poses)
        step_rows, step_starts = FR.time_steps(times)
        d = [up(x) for x in (poses, cov, times, step_rows, step_starts)]
        empty, table = FR.new_track_table(CAPACITY, NJ, dev), FR.new_track_table(CAPACITY, NJ, dev)
        i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)
        out = [i32(n), i32(n), torch.empty(n, device=dev), i32(n), i32(CAPACITY + 1), i32(1), i32(1)]
        ws = torch.empty(lib.metro_associate_tracks_workspace_bytes(CAPACITY, NJ), dtype=torch.uint8, device=dev)

        def reset():
            for t, e in zip(table, empty):
                t.copy_(e)

        def launch():
            reset()
            _lib.check(lib.metro_associate_tracks(p(d[0]), p(d[1]), p(d[2]), n, p(d[3]), n, p(d[4]), n_frames, C.byref(cs),
                                                  _lib.METRO_SMOOTH_COVARIANCE, 4e6, 1.0, 1.0, 2000.0, 0.0, 300.0, 600.0, 9, 1.0,
                                                  p(table.state), CAPACITY, p(table.ids), p(table.next_id), p(ws), *[p(o) for o in out],
                                                  stream), 'metro_associate_tracks')
        key = f'associate_{n_tracks}x{n_frames}'
        result[key + '_with_reset_us'] = windows_us(launch, windows, iters)
        result[key + '_reset_us'] = windows_us(reset, windows, iters)
        assert int(out[5].item()) == n_tracks and int(out[6].item()) == 0 and int(table.next_id.item()) == n_tracks, 'every box continues its track'

    n_tracks, n_frames = 8, 8
    spec = ModelSpec(50, 32, 'h36m')
    boxes = np.array([[120.0 + 210 * q + 6 * f, 200.0 + 40 * (q % 3) + 3 * f, 180.0, 520.0] for f in range(n_frames) for q in range(n_tracks)])
    fi, ti = np.repeat(np.arange(n_frames), n_tracks), np.tile(np.arange(n_tracks), n_frames)
    depth, stamps = 3000.0 + 1000.0 * ti, np.arange(n_frames) / FPS
    result['scene'] = (f'{n_tracks} tracks x {n_frames} frames = {len(boxes)} boxes at {FPS:g} fps, J = {NJ}; RN50 stride 32 h36m (synthetic weights), '
                       'f16, true-root-depth; 1920x1080 uint8 frames and boxes on the device (geometry=device)')
    params = synth.make_params(spec.arch, spec.n_head_channels, spec.base_width, seed=0, logit_gain=synth.logit_gain_for(50, 32))
    frames = [torch.from_numpy(rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8)).to(dev) for _ in range(n_frames)]
    d_boxes = torch.from_numpy(boxes).to(dev)
    cam = Camera(np.array([[1500.0, 0, 960], [0, 1500.0, 540], [0, 0, 1]]))
    kw = dict(scale_recovery='true-root-depth', root_depth=depth, precision='f16')
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'rn50_s32.npz')
        save_model(path, spec, params)
        track = lambda: FR.track_poses_in_frames(frames, d_boxes, path, cam, ti, fi, stamps, **kw)
        follow = lambda: FR.follow_poses_in_frames(frames, d_boxes, path, cam, fi, stamps, capacity=CAPACITY, **kw)
        result['calls_per_s'] = interleaved_calls_per_s((('track', track), ('follow', follow), ('track_again', track)), windows, calls)
    text = json.dumps(result, indent=1, sort_keys=True)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
