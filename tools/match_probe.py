#!/usr/bin/env python3
"""What matching persons across cameras costs: the metro_view_affinity and metro_cluster_views launches, and the whole
match_poses_in_frames call next to triangulate_poses_in_frames given the true person_index.

    python tools/match_probe.py [--out FILE] [--quick]          # one JSON object on stdout (and in FILE, default
                                                                # profiles/match_probe.json)

Persons seen by 4 cameras on a ring, RN50 stride 32 h36m (J = 17, synthetic weights), f16; frames (1920 x 1080 uint8) and boxes
on the device, boxes camera by camera as a detector gives them.
  * us per launch at 64 boxes (16 persons) and at 128 boxes (32 persons), on rays that meet (coords01 projected through the
    crop records, so every person's boxes merge: 48 and 96 rounds of the clustering loop, its longest run short of a scene
    whose boxes all join): metro_view_affinity in both weight modes and metro_cluster_views at max_cost 200 mm; device events
    around 200 back-to-back launches of the C entry after 20 warm-up launches, median of 5 windows.  The clustering is checked
    to recover the persons;
  * calls/s of match_poses_in_frames against triangulate_poses_in_frames with the true person_index on the same 64 boxes
    (covariance weights both).  Three arms INTERLEAVED window by window in one process: triangulate, match, triangulate
    again.  The two triangulate arms are the same code on the same data: their relative difference (`aa_spread`) is the
    noise margin the match arm has to be read against.  Host clock around `calls` calls (each ends in its own
    synchronisation), after 3 warm-up windows, median of 5 windows.  With synthetic weights the forward's rays do not meet, so
    the match arm's clustering stops after few rounds; the launch figures above are the ones for a scene that merges.
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
from metro_pose3d_amd import heads as MH  # noqa: E402

ANGLES = (0.0, 85.0, 170.0, 265.0)
MAX_COST_MM, CLIP_MM = 200.0, 500.0


def rig(spec, n_persons, rng):
    """-> (cameras, boxes [4 P, 4] camera-major, frame_index, person_index, coords01 [4 P, J_head, 3] whose rays meet, records)."""
    centre = np.array([0.0, 0.0, 1000.0])
    cams = []
    for k, ang in enumerate(np.radians(ANGLES)):
        t = centre + np.array([4500 * np.cos(ang), 4500 * np.sin(ang), 300.0])
        z = (centre - t) / np.linalg.norm(centre - t)
        x = np.cross(z, [0.0, 0.0, 1.0])
        x /= np.linalg.norm(x)
        dist = np.float32([-0.12, 0.04, 0.001, -0.0015, 0.005]) if k % 2 else None
        cams.append(FR.Camera(np.array([[1150.0, 0, 960], [0, 1150.0, 540], [0, 0, 1]]), dist, R=np.stack([x, np.cross(z, x), z]), t=t))
    sk = spec.skeleton
    side = int(np.ceil(np.sqrt(n_persons)))
    grid = np.array([[(p % side) - (side - 1) / 2, (p // side) - (side - 1) / 2, 0.0] for p in range(n_persons)]) * (2400.0 / side)
    joints = centre + grid[:, None, :] + rng.normal(0, 300, (n_persons, sk.n_out, 3))
    boxes, fi, pi = [], [], []
    for c, cam in enumerate(cams):
        for p in range(n_persons):
            xc = (joints[p] - cam.t.astype(np.float64)) @ cam.R.astype(np.float64).T
            px = xc[:, :2] / xc[:, 2:] * 1150.0 + [960.0, 540.0]
            lo, hi = px.min(axis=0) - 30, px.max(axis=0) + 30
            boxes.append([lo[0], lo[1], hi[0] - lo[0], hi[1] - lo[1]])
            fi.append(c)
            pi.append(p)
    boxes, fi, pi = np.array(boxes), np.array(fi), np.array(pi)
    q = FR.placement_params(cams, boxes, fi, spec.proc_side)
    last = spec.proc_side - 1
    lrc, half = last - last % spec.stride - 1, spec.stride // 2 if spec.centered_stride else 0
    coords01 = np.zeros((len(boxes), sk.n_head, 3), np.float32)
    for i in range(len(boxes)):
        xv = (joints[pi[i]] - q.cam_loc[i].astype(np.float64)) @ q.rot_to_world[i].astype(np.float64)
        px = xv @ np.linalg.inv(q.inv_intrinsics[i].astype(np.float64)).T
        coords01[i, list(sk.permutation), :2] = (px[:, :2] / px[:, 2:] - half) / lrc
    return cams, boxes, fi, pi, coords01, q


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
    a = 0.5 * (med['triangulate'] + med['triangulate_again'])
    out = {k: {'median': round(med[k], 2), 'windows': [round(v, 2) for v in res[k]]} for k in res}
    out['aa_spread'] = round(abs(med['triangulate'] - med['triangulate_again']) / a, 4)
    out['match_over_triangulate'] = round(med['match'] / a, 4)
    return out


def launches(spec, n_persons, dev, rng, windows, iters):
    """The two launches on a rig of n_persons -> their timings; the clustering must recover the persons."""
    sk = spec.skeleton
    cams, boxes, fi, pi, coords01, q = rig(spec, n_persons, rng)
    n = len(boxes)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_c01, d_places, d_fi = up(coords01), up(FR.pack_placements(q)).reshape(-1), up(fi.astype(np.int32))
    d_cov = up(np.tile(np.float32([4e-5, 4e-5, 1e-3, 0, 0, 0]), (n, sk.n_head, 1)) * rng.uniform(0.5, 4, (n, sk.n_head, 1)).astype(np.float32))
    mirror = up(np.asarray(sk.out_mirror, np.int32))
    cost = torch.empty((n, n), device=dev)
    n_pairs = torch.empty((n, n), dtype=torch.int32, device=dev)
    i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)
    labels, n_found, rows, starts = i32(n), i32(1), i32(n), i32(n + 1)
    lib, stream, cs = _lib.load(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), spec.to_c(1)
    p = lambda x: C.c_void_p(x.data_ptr())
    min_sin2, min_pairs = float(np.sin(np.radians(2.0)) ** 2), (sk.n_out + 1) // 2
    out = {'boxes': n, 'persons': n_persons}
    for weights in ('uniform', 'covariance'):
        launch = lambda: _lib.check(lib.metro_view_affinity(
            p(d_c01), p(d_cov), p(d_places), C.byref(cs), p(mirror), p(d_fi), n, 1, MH.TRI_WEIGHTS[weights], min_sin2, CLIP_MM,
            min_pairs, p(cost), p(n_pairs), stream), 'metro_view_affinity')
        out[f'view_affinity_us_{weights}'] = launch_us(launch, windows, iters)
    launch = lambda: _lib.check(lib.metro_cluster_views(p(cost), n, 1, MAX_COST_MM, p(labels), p(n_found), p(rows), p(starts), stream),
                                'metro_cluster_views')
    out['cluster_views_us'] = launch_us(launch, windows, iters)
    assert int(n_found.item()) == n_persons and np.array_equal(labels.cpu().numpy(), pi), 'the probe scene must cluster into its persons'
    out['merges'] = n - n_persons
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'match_probe.json'), help='where the JSON object is written')
    ap.add_argument('--quick', action='store_true', help='fewer windows (under a profiler)')
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('match_probe: no HIP device (these numbers exist only on the GPU)')
    windows, iters, calls = (1, 20, 2) if opts.quick else (5, 200, 10)
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    spec = ModelSpec(50, 32, 'h36m')
    result = {'device': torch.cuda.get_device_name(dev),
              'scene': f'persons x {len(ANGLES)} cameras, J = {spec.skeleton.n_out}; RN50 stride 32 h36m (synthetic weights), f16; '
                       '1920x1080 uint8 frames and boxes on the device (geometry=device), cameras 1 and 3 distorted'}
    result['launches_64_boxes'] = launches(spec, 16, dev, rng, windows, iters)
    result['launches_128_boxes'] = launches(spec, 32, dev, rng, windows, iters)

    cams, boxes, fi, pi, _, _ = rig(spec, 16, rng)
    params = synth.make_params(spec.arch, spec.n_head_channels, spec.base_width, seed=0, logit_gain=synth.logit_gain_for(50, 32))
    frames = [torch.from_numpy(rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8)).to(dev) for _ in cams]
    d_boxes = torch.from_numpy(boxes).to(dev)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'rn50_s32.npz')
        save_model(path, spec, params)
        triangulate = lambda: FR.triangulate_poses_in_frames(frames, d_boxes, path, cams, pi, fi, precision='f16')
        match = lambda: FR.match_poses_in_frames(frames, d_boxes, path, cams, fi, precision='f16')
        result['calls_per_s_64_boxes'] = interleaved_calls_per_s(
            (('triangulate', triangulate), ('match', match), ('triangulate_again', triangulate)), windows, calls)
        result['persons_found_by_the_synthetic_forward'] = int(match().world.poses.shape[0])
    text = json.dumps(result, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
