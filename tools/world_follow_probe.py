#!/usr/bin/env python3
"""What following persons through several cameras over video costs: the three launches follow_world_poses_in_frames adds
(metro_view_affinity_steps, metro_triangulate_joints_cov, metro_person_steps), and the whole call next to
match_poses_in_frames on the same boxes.

    python tools/world_follow_probe.py [--out FILE] [--quick]   # one JSON object on stdout (and in FILE, default
                                                                # profiles/world_follow_probe.json)

16 persons seen by 4 cameras on a ring at 2 time steps: 128 boxes, RN50 stride 32 h36m (J = 17, synthetic weights), f16; frames
(1920 x 1080 uint8, one per camera and step) and boxes on the device, boxes step by step and camera by camera.
  * us per launch on rays that meet (tools/match_probe.py's rig, the second step a copy of the first): the gated affinity and
    the covariance triangulation in both weight modes and metro_person_steps; device events around 200 back-to-back launches
    of the C entry after 20 warm-up launches, median of 5 windows.  The clustering is checked to find 32 persons, 16 per step;
  * calls/s of follow_world_poses_in_frames against match_poses_in_frames on the same 128 boxes.  Three arms INTERLEAVED window
    by window in one process: match, follow, match again.  The two match arms are the same code on the same data: their
    relative difference (`aa_spread`) is the noise margin the follow arm has to be read against.  Host clock around `calls`
    calls (each ends in its own synchronisation), after 3 warm-up windows, median of 5 windows.  With synthetic weights the
    forward's rays do not meet, so few boxes merge in either arm; the launch figures above are the ones for a scene that does.
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
from match_probe import ANGLES, CLIP_MM, MAX_COST_MM, launch_us, rig  # noqa: E402

PERSONS, STEPS = 16, 2


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
    a = 0.5 * (med['match'] + med['match_again'])
    out = {k: {'median': round(med[k], 2), 'windows': [round(v, 2) for v in res[k]]} for k in res}
    out['aa_spread'] = round(abs(med['match'] - med['match_again']) / a, 4)
    out['follow_over_match'] = round(med['follow'] / a, 4)
    return out


def launches(spec, dev, rng, windows, iters):
    sk = spec.skeleton
    cams, boxes, fi, pi, coords01, q = rig(spec, PERSONS, rng)
    one = len(boxes)
    n = one * STEPS
    twice = lambda a: np.concatenate([a] * STEPS)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    q = type(q)(*(twice(a) for a in q))
    fi = np.concatenate([fi + len(cams) * t for t in range(STEPS)]).astype(np.int32)
    step = np.repeat(np.arange(STEPS), one).astype(np.int32)
    d_c01, d_places, d_fi, d_step = up(twice(coords01)), up(FR.pack_placements(q)).reshape(-1), up(fi), up(step)
    d_cov = up(np.tile(np.float32([4e-5, 4e-5, 1e-3, 0, 0, 0]), (n, sk.n_head, 1)) * rng.uniform(0.5, 4, (n, sk.n_head, 1)).astype(np.float32))
    mirror = up(np.asarray(sk.out_mirror, np.int32))
    cost = torch.empty((n, n), device=dev)
    n_pairs = torch.empty((n, n), dtype=torch.int32, device=dev)
    lib, stream, cs = _lib.load(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), spec.to_c(1)
    p = lambda x: C.c_void_p(x.data_ptr())
    min_sin2, min_pairs = float(np.sin(np.radians(2.0)) ** 2), (sk.n_out + 1) // 2
    out = {'boxes': n, 'persons_per_step': PERSONS, 'steps': STEPS}
    for weights in ('uniform', 'covariance'):
        launch = lambda: _lib.check(lib.metro_view_affinity_steps(
            p(d_c01), p(d_cov), p(d_places), C.byref(cs), p(mirror), p(d_fi), p(d_step), n, 1, MH.TRI_WEIGHTS[weights], min_sin2,
            CLIP_MM, min_pairs, p(cost), p(n_pairs), stream), 'metro_view_affinity_steps')
        out[f'view_affinity_steps_us_{weights}'] = launch_us(launch, windows, iters)
    labels, n_found, rows, starts = MH.cluster_views(cost, MAX_COST_MM)
    assert int(n_found.item()) == PERSONS * STEPS, 'the probe scene must cluster into its persons, step by step'
    assert np.array_equal(labels.cpu().numpy(), np.concatenate([pi + PERSONS * t for t in range(STEPS)]))
    points = torch.empty((n, sk.n_out, 3), device=dev)
    n_rays = torch.empty((n, sk.n_out), dtype=torch.int32, device=dev)
    residual = torch.empty((n, sk.n_out), device=dev)
    cov = torch.empty((n, sk.n_out, 9), device=dev)
    for weights in ('uniform', 'covariance'):
        launch = lambda: _lib.check(lib.metro_triangulate_joints_cov(
            p(d_c01), p(d_cov), p(d_places), n, p(rows), rows.numel(), p(starts), n, C.byref(cs), p(mirror), MH.TRI_WEIGHTS[weights],
            float(np.sin(np.radians(2.0)) ** 2 / 4), p(points), p(n_rays), p(residual), p(cov), stream), 'metro_triangulate_joints_cov')
        out[f'triangulate_joints_cov_us_{weights}'] = launch_us(launch, windows, iters)
    times = up(np.arange(STEPS) / 32.0)
    i32 = lambda k: torch.empty(k, dtype=torch.int32, device=dev)
    person_step, step_rows, step_starts = i32(n), i32(n), i32(STEPS + 1)
    person_times = torch.empty(n, dtype=torch.float64, device=dev)
    launch = lambda: _lib.check(lib.metro_person_steps(
        p(rows), rows.numel(), p(starts), p(n_found), n, 1, p(d_step), n, p(times), STEPS, p(person_step), p(person_times), p(step_rows),
        p(step_starts), stream), 'metro_person_steps')
    out['person_steps_us'] = launch_us(launch, windows, iters)
    assert step_starts.tolist() == [0, PERSONS, PERSONS * STEPS]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'world_follow_probe.json'), help='where the JSON object is written')
    ap.add_argument('--quick', action='store_true', help='fewer windows (under a profiler)')
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('world_follow_probe: no HIP device (these numbers exist only on the GPU)')
    windows, iters, calls = (1, 20, 2) if opts.quick else (5, 200, 10)
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    spec = ModelSpec(50, 32, 'h36m')
    result = {'device': torch.cuda.get_device_name(dev),
              'scene': f'{PERSONS} persons x {len(ANGLES)} cameras x {STEPS} steps, J = {spec.skeleton.n_out}; RN50 stride 32 h36m '
                       '(synthetic weights), f16; 1920x1080 uint8 frames and boxes on the device (geometry=device), cameras 1 and 3 distorted'}
    result['launches_128_boxes'] = launches(spec, dev, rng, windows, iters)

    cams, boxes, fi, _, _, _ = rig(spec, PERSONS, rng)
    params = synth.make_params(spec.arch, spec.n_head_channels, spec.base_width, seed=0, logit_gain=synth.logit_gain_for(50, 32))
    frames = [torch.from_numpy(rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8)).to(dev) for _ in range(len(cams) * STEPS)]
    d_boxes = torch.from_numpy(np.concatenate([boxes] * STEPS)).to(dev)
    fi = np.concatenate([fi + len(cams) * t for t in range(STEPS)])
    stamps = np.repeat(np.arange(STEPS) / 32.0, len(cams))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'rn50_s32.npz')
        save_model(path, spec, params)
        match = lambda: FR.match_poses_in_frames(frames, d_boxes, path, cams * STEPS, fi, precision='f16')
        follow = lambda: FR.follow_world_poses_in_frames(frames, d_boxes, path, cams * STEPS, fi, stamps, precision='f16')
        result['calls_per_s_128_boxes'] = interleaved_calls_per_s((('match', match), ('follow', follow), ('match_again', match)),
                                                                  windows, calls)
        result['persons_found_by_the_synthetic_forward'] = int(follow().world.poses.shape[0])
    text = json.dumps(result, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
