#!/usr/bin/env python3
"""What learning the bone lengths of followed persons costs: the metro_track_bone_lengths launch, and Follower.follow on a rig with
and without learn_bones.

    python tools/bone_lengths_probe.py [--out FILE] [--quick]   # one JSON object on stdout (and in FILE, default
                                                                # profiles/bone_lengths_probe.json)

  * us per launch at 16 tracks x 8 rows and at 128 tracks x 64 rows (J = 17, the 16 h36m edges, covariance mode, the defaults of
    heads.track_bone_lengths): every track a rigid skeleton in rigid motion with joint noise of a few mm and a matching
    covariance; device events around 200 back-to-back launches of the C entry after 20 warm-up launches, median of 5 windows.
    The launches accumulate into one table (the walk per row does not depend on what the table holds); it is checked afterwards
    that every (slot, bone) pair is known.  Next to it the read-out alone (n_rows = 0) at both table sizes.
  * calls/s of Follower(world=True).follow on tools/match_probe.py's rig (16 persons x 4 cameras, one exposure, 64 boxes, RN50
    stride 32 h36m with synthetic weights, f16, 1920x1080 uint8 frames and boxes on the device) without and with learn_bones.
    Three arms INTERLEAVED window by window in one process: off, on, off again.  The two off arms are the same code on the same
    data: their relative difference (`aa_spread`) is the noise margin the on arm has to be read against.  Host clock around
    `calls` calls (each ends in its own synchronisation), after 3 warm-up windows, median of 5 windows.
No time is fixed in advance: the figures are what the probe reports."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from metro_pose3d_amd import ModelSpec, _lib, save_model, synth  # noqa: E402
from metro_pose3d_amd import frames as FR  # noqa: E402
from metro_pose3d_amd import heads as MH  # noqa: E402
from match_probe import ANGLES, launch_us, rig  # noqa: E402

PERSONS = 16
SIZES = ((16, 8), (128, 64))


def tracks_scene(sk, n_tracks, n_rows, rng):
    """-> (poses fp32 [T S, J, 3], cov fp32 [T S, J, 9], rows int32 [T S], starts int32 [T + 1]); row s T + t is track t at step s."""
    base = rng.normal(0, 250, (n_tracks, sk.n_out, 3))
    poses, cov = np.empty((n_rows, n_tracks, sk.n_out, 3)), np.empty((n_rows, n_tracks, sk.n_out, 3, 3))
    for s in range(n_rows):
        for t in range(n_tracks):
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            a = rng.normal(0, rng.uniform(2, 8), (sk.n_out, 3, 3))
            cov[s, t] = a @ a.transpose(0, 2, 1) + np.eye(3)
            noise = np.einsum('jab,jb->ja', np.linalg.cholesky(cov[s, t]), rng.normal(size=(sk.n_out, 3)))
            poses[s, t] = base[t] @ q.T + rng.normal(0, 2000, 3) + noise
    rows = (np.arange(n_rows)[None, :] * n_tracks + np.arange(n_tracks)[:, None]).reshape(-1)
    starts = np.arange(n_tracks + 1) * n_rows
    return (poses.reshape(-1, sk.n_out, 3).astype(np.float32), cov.reshape(-1, sk.n_out, 9).astype(np.float32), rows.astype(np.int32),
            starts.astype(np.int32))


def launches(sk, dev, rng, windows, iters):
    lib, stream = _lib.load(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    p = lambda x: C.c_void_p(x.data_ptr() if x is not None else 0)
    edges, mirror = up(np.asarray(sk.edges, np.int32)), up(np.asarray(sk.edge_mirror(), np.int32))
    n_edges = len(sk.edges)
    out = {}
    for n_tracks, n_rows in SIZES:
        poses, cov, rows, starts = (up(a) for a in tracks_scene(sk, n_tracks, n_rows, rng))
        table = FR.new_bone_table(n_tracks, n_edges, dev)
        ids = torch.arange(n_tracks, dtype=torch.int32, device=dev)
        lengths, sigma = (torch.empty((n_tracks, n_edges), dtype=torch.float64, device=dev) for _ in range(2))
        known = torch.empty((n_tracks, n_edges), dtype=torch.uint8, device=dev)
        tail = (p(ids), sk.n_out, p(edges), p(mirror), n_edges, None, *MH.bone_length_params(), p(table.stats), p(table.ids), p(lengths),
                p(sigma), p(known), stream)
        walk = lambda: _lib.check(lib.metro_track_bone_lengths(p(poses), p(cov), len(poses), p(rows), len(rows), p(starts), n_tracks, *tail),
                                  'metro_track_bone_lengths')
        read = lambda: _lib.check(lib.metro_track_bone_lengths(None, None, 0, None, 0, None, n_tracks, *tail), 'metro_track_bone_lengths')
        key = f'{n_tracks}x{n_rows}'
        out[f'track_bone_lengths_us_{key}'] = launch_us(walk, windows, iters)
        out[f'read_out_us_{key}'] = launch_us(read, windows, iters)
        assert bool(known.all()) and bool(torch.isfinite(lengths).all()), 'every bone of every track must be known after the walk'
        out[f'rejected_share_{key}'] = round(float(table.stats[..., 3].sum() / (table.stats[..., 2].sum() + table.stats[..., 3].sum())), 4)
    return out


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
    a = 0.5 * (med['off'] + med['off_again'])
    out = {k: {'median': round(med[k], 2), 'windows': [round(v, 2) for v in res[k]]} for k in res}
    out['aa_spread'] = round(abs(med['off'] - med['off_again']) / a, 4)
    out['on_over_off'] = round(med['on'] / a, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bone_lengths_probe.json'), help='where the JSON object is written')
    ap.add_argument('--quick', action='store_true', help='fewer windows (under a profiler)')
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bone_lengths_probe: no HIP device (these numbers exist only on the GPU)')
    windows, iters, calls = (1, 20, 2) if opts.quick else (5, 200, 10)
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    spec = ModelSpec(50, 32, 'h36m')
    result = {'device': torch.cuda.get_device_name(dev),
              'scene': f'launches: tracks x rows {SIZES}, J = {spec.skeleton.n_out}, {len(spec.skeleton.edges)} h36m edges, covariance mode; '
                       f'calls: {PERSONS} persons x {len(ANGLES)} cameras, one exposure; RN50 stride 32 h36m (synthetic weights), f16; '
                       '1920x1080 uint8 frames and boxes on the device (geometry=device), cameras 1 and 3 distorted'}
    result['launches'] = launches(spec.skeleton, dev, rng, windows, iters)

    cams, boxes, fi, _, _, _ = rig(spec, PERSONS, rng)
    params = synth.make_params(spec.arch, spec.n_head_channels, spec.base_width, seed=0, logit_gain=synth.logit_gain_for(50, 32))
    frames = [torch.from_numpy(rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8)).to(dev) for _ in cams]
    d_boxes, stamps = torch.from_numpy(boxes).to(dev), np.zeros(len(cams))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'rn50_s32.npz')
        save_model(path, spec, params)
        off = FR.Follower(path, cams, world=True, single_view='rays', precision='f16')
        on = FR.Follower(path, cams, world=True, single_view='rays', learn_bones=True, precision='f16')
        arms = (('off', lambda: off.follow(frames, d_boxes, fi, stamps)), ('on', lambda: on.follow(frames, d_boxes, fi, stamps)),
                ('off_again', lambda: off.follow(frames, d_boxes, fi, stamps)))
        result['calls_per_s'] = interleaved_calls_per_s(arms, windows, calls)
        last = on.follow(frames, d_boxes, fi, stamps)
        result['synthetic_forward'] = {'persons': int(last.world.poses.shape[0]), 'tracked': int((last.track_index >= 0).sum()),
                                       'lengths_accepted': int(on.bones.stats[..., 2].sum())}
    text = json.dumps(result, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
