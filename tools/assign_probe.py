#!/usr/bin/env python3
"""What the optimal box-to-track assignment costs next to the greedy one: us per launch of metro_associate_tracks and of
metro_associate_tracks_optimal on the same inputs.

    python tools/assign_probe.py [--out FILE] [--quick]          # one JSON object on stdout (and in FILE)

J = 17, covariance measurements, from an empty table each time (the table is reset by three small device copies inside the
timed window, which are timed on their own as `reset_us`).
  * 8 tracks x 8 frames and 16 tracks x 64 frames (capacity 64): tools/follow_probe.py's scenes, persons on a 1 m grid
    drifting a few mm a frame, so every row of a step's cost matrix has one admissible column;
  * crowded: 128 tracks x 8 frames (capacity 128), persons of one build on a line 150 mm apart drifting a few mm a frame, so
    most rows have three admissible columns (the person and both neighbours).
Three arms INTERLEAVED window by window in one process: greedy, optimal, greedy again.  The two greedy arms are the same code on
the same data: their relative difference (`aa_spread`) is the noise margin the optimal arm has to be read against.  Device
events around back-to-back launches of the C entry after 20 warm-up launches per arm, median of 5 windows.
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

FPS, NJ = 32.0, 17


def grid_scene(rng, n_tracks, n_frames):
    """tools/follow_probe.py's scene -> (poses [n, J, 3], cov [n, J, 9], times [n]), frame-major."""
    cloud = rng.uniform(-300, 300, (n_tracks, NJ, 3))
    v = rng.uniform(-8, 8, (n_tracks, 1, 3))
    centre = np.stack([1000.0 * (np.arange(n_tracks) % 4), 1000.0 * (np.arange(n_tracks) // 4), np.full(n_tracks, 3000.0)], 1)[:, None]
    poses = np.concatenate([centre + cloud + v * f + rng.normal(0, 2, cloud.shape) for f in range(n_frames)]).astype(np.float32)
    return poses, _cov(rng, len(poses)), np.repeat(np.arange(n_frames) / FPS, n_tracks)


def crowded_scene(rng, n_tracks, n_frames, spacing=150.0):
    """Persons of one build (one joint cloud) on a line `spacing` mm apart: a neighbour's box costs about `spacing`."""
    cloud = rng.uniform(-300, 300, (1, NJ, 3))
    v = rng.uniform(-8, 8, (n_tracks, 1, 3))
    centre = np.stack([spacing * np.arange(n_tracks), np.zeros(n_tracks), np.full(n_tracks, 3000.0)], 1)[:, None]
    poses = np.concatenate([centre + cloud + v * f + rng.normal(0, 2, (n_tracks, NJ, 3)) for f in range(n_frames)]).astype(np.float32)
    return poses, _cov(rng, len(poses)), np.repeat(np.arange(n_frames) / FPS, n_tracks)


def _cov(rng, n):
    a = rng.normal(size=(n, NJ, 3, 3))
    return (a @ a.transpose(0, 1, 3, 2) * 3 + 4 * np.eye(3)).astype(np.float32).reshape(n, NJ, 9)


def interleaved_us(arms, windows, iters):
    for _, fn in arms:
        for _ in range(20):
            fn()
    res = {k: [] for k, _ in arms}
    for _ in range(windows):
        for name, fn in arms:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            res[name].append(a.elapsed_time(b) * 1e3 / iters)
    return {k: {'median': round(statistics.median(v), 2), 'windows': [round(x, 2) for x in v]} for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the JSON object to this file')
    ap.add_argument('--quick', action='store_true', help='fewer windows (under a profiler)')
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('assign_probe: no HIP device (these numbers exist only on the GPU)')
    windows, iters = (1, 5) if opts.quick else (5, 50)
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    result = {'device': torch.cuda.get_device_name(dev)}
    lib, stream = _lib.load(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    p = lambda x: C.c_void_p(x.data_ptr())
    cs = _lib.MetroSpec(n_joints_out=NJ)
    for key, scene, n_tracks, n_frames, capacity in (('8x8', grid_scene, 8, 8, 64), ('16x64', grid_scene, 16, 64, 64),
                                                     ('crowded_128x8', crowded_scene, 128, 8, 128)):
        poses, cov, times = scene(rng, n_tracks, n_frames)
        n = len(poses)
        step_rows, step_starts = FR.time_steps(times)
        d = [up(x) for x in (poses, cov, times, step_rows, step_starts)]
        empty, table = FR.new_track_table(capacity, NJ, dev), FR.new_track_table(capacity, NJ, dev)
        i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)
        out = [i32(n), i32(n), torch.empty(n, device=dev), i32(n), i32(capacity + 1), i32(1), i32(1)]
        ws = torch.empty(lib.metro_associate_tracks_workspace_bytes(capacity, NJ), dtype=torch.uint8, device=dev)

        def reset():
            for t, e in zip(table, empty):
                t.copy_(e)

        def launch(entry):
            reset()
            _lib.check(getattr(lib, entry)(p(d[0]), p(d[1]), p(d[2]), n, p(d[3]), n, p(d[4]), n_frames, C.byref(cs),
                                           _lib.METRO_SMOOTH_COVARIANCE, 4e6, 1.0, 1.0, 2000.0, 0.0, 300.0, 600.0, 9, 1.0, p(table.state),
                                           capacity, p(table.ids), p(table.next_id), p(ws), *[p(o) for o in out], stream), entry)
        greedy, optimal = (lambda: launch('metro_associate_tracks')), (lambda: launch('metro_associate_tracks_optimal'))
        pairs = {}
        for name, fn in (('greedy', greedy), ('optimal', optimal)):
            fn()
            pairs[name] = {'new': int(out[5].item()), 'dropped': int(out[6].item()), 'continued': int((~torch.isnan(out[2])).sum().item())}
            assert pairs[name]['new'] == n_tracks and pairs[name]['dropped'] == 0, 'every box continues its track'
        r = interleaved_us((('greedy', greedy), ('optimal', optimal), ('greedy_again', greedy), ('reset', reset)), windows, iters)
        a = 0.5 * (r['greedy']['median'] + r['greedy_again']['median'])
        result[key] = {'boxes': n, 'capacity': capacity, 'decisions': pairs, 'with_reset_us': {k: r[k] for k in ('greedy', 'optimal', 'greedy_again')},
                       'reset_us': r['reset'], 'aa_spread': round(abs(r['greedy']['median'] - r['greedy_again']['median']) / a, 4),
                       'optimal_over_greedy': round(r['optimal']['median'] / a, 4)}
    text = json.dumps(result, indent=1, sort_keys=True)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
