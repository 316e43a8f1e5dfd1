#!/usr/bin/env python3
"""What triangulating costs: the metro_triangulate_joints launch, and the whole multi-camera call next to the nearest
single-camera one.

    python tools/triangulate_probe.py [--out FILE] [--quick]          # one JSON object on stdout (and in FILE)

16 persons seen by 4 cameras on a ring (64 boxes), RN50 stride 32 h36m (J = 17, synthetic weights), f16; frames (1920 x 1080
uint8) and boxes on the device, so no per-box host geometry hides the launches.
  * us per metro_triangulate_joints launch in both weight modes, on rays that meet (coords01 projected through the crop
    records, so every joint runs both passes and the residual): device events around 200 back-to-back launches of the C entry
    after 20 warm-up launches, median of 5 windows;
  * calls/s of triangulate_poses_in_frames (covariance weights) against locate_poses_in_frames(scale_recovery='metro',
    return_uncertainty=True) on the same frames and boxes -- the same warp and moments forward, then place_poses + merge +
    place_covariances there, triangulate + place_poses + merge here.  Three arms INTERLEAVED window by window in one
    process: locate, triangulate, locate again.  The two locate arms are the same code on the same data: their relative
    difference (`aa_spread`) is the noise margin the triangulate arm has to be read against.  Host clock around `calls` calls
    (each ends in its own synchronisation), after 3 warm-up windows, median of 5 windows.
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

N_PERSONS, ANGLES = 16, (0.0, 85.0, 170.0, 265.0)


def rig(spec, rng):
    """-> (cameras, boxes [64, 4], frame_index, person_index, coords01 [64, J_head, 3] whose rays meet, placement records)."""
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
    joints = centre + rng.uniform(-900, 900, (N_PERSONS, 1, 3)) * [1, 1, 0.2] + rng.normal(0, 250, (N_PERSONS, sk.n_out, 3))
    boxes, fi, pi = [], [], []
    for p in range(N_PERSONS):
        for c, cam in enumerate(cams):
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
    a = 0.5 * (med['locate'] + med['locate_again'])
    out = {k: {'median': round(med[k], 2), 'windows': [round(v, 2) for v in res[k]]} for k in res}
    out['aa_spread'] = round(abs(med['locate'] - med['locate_again']) / a, 4)
    out['triangulate_over_locate'] = round(med['triangulate'] / a, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='also write the JSON object to this file')
    ap.add_argument('--quick', action='store_true', help='fewer windows (under a profiler)')
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('triangulate_probe: no HIP device (these numbers exist only on the GPU)')
    windows, iters, calls = (1, 20, 2) if opts.quick else (5, 200, 10)
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    spec = ModelSpec(50, 32, 'h36m')
    sk = spec.skeleton
    cams, boxes, fi, pi, coords01, q = rig(spec, rng)
    n = len(boxes)
    result = {'device': torch.cuda.get_device_name(dev),
              'scene': f'{N_PERSONS} persons x {len(cams)} cameras = {n} boxes, J = {sk.n_out}; RN50 stride 32 h36m (synthetic '
                       'weights), f16; 1920x1080 uint8 frames and boxes on the device (geometry=device), cameras 1 and 3 distorted'}

    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_c01, d_places = up(coords01), up(FR.pack_placements(q)).reshape(-1)
    d_cov = up(np.tile(np.float32([4e-5, 4e-5, 1e-3, 0, 0, 0]), (n, sk.n_head, 1)) * rng.uniform(0.5, 4, (n, sk.n_head, 1)).astype(np.float32))
    rows, starts = FR.person_groups(pi, fi)
    d_rows, d_starts = up(rows), up(starts)
    mirror = up(np.asarray(sk.out_mirror, np.int32))
    pts = torch.empty((N_PERSONS, sk.n_out, 3), device=dev)
    cnt = torch.empty((N_PERSONS, sk.n_out), dtype=torch.int32, device=dev)
    res = torch.empty((N_PERSONS, sk.n_out), device=dev)
    lib, stream, cs = _lib.load(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), spec.to_c(1)
    p = lambda x: C.c_void_p(x.data_ptr())
    min_det = MH.triangulation_min_det('covariance', 2.0)
    for weights in ('uniform', 'covariance'):
        launch = lambda: _lib.check(lib.metro_triangulate_joints(
            p(d_c01), p(d_cov), p(d_places), n, p(d_rows), len(rows), p(d_starts), N_PERSONS, C.byref(cs), p(mirror),
            MH.TRI_WEIGHTS[weights], min_det, p(pts), p(cnt), p(res), stream), 'metro_triangulate_joints')
        result[f'triangulate_joints_us_{weights}'] = launch_us(launch, windows, iters)
        assert int(cnt.min()) == len(cams) and bool(torch.isfinite(pts).all()), 'the probe rays must all enter the solve'
    result['triangulate_joints_worst_residual_mm'] = round(float(res.max()), 6)

    params = synth.make_params(spec.arch, spec.n_head_channels, spec.base_width, seed=0, logit_gain=synth.logit_gain_for(50, 32))
    frames = [torch.from_numpy(rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8)).to(dev) for _ in cams]
    d_boxes = torch.from_numpy(boxes).to(dev)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'rn50_s32.npz')
        save_model(path, spec, params)
        locate = lambda: FR.locate_poses_in_frames(frames, d_boxes, path, cameras=cams, frame_index=fi, scale_recovery='metro',
                                                   coords='world', precision='f16', return_uncertainty=True)
        triangulate = lambda: FR.triangulate_poses_in_frames(frames, d_boxes, path, cams, pi, fi, precision='f16')
        result['calls_per_s'] = interleaved_calls_per_s((('locate', locate), ('triangulate', triangulate), ('locate_again', locate)),
                                                        windows, calls)
    text = json.dumps(result, indent=1, sort_keys=True)
    if opts.out:
        os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
        with open(opts.out, 'w') as f:
            f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
