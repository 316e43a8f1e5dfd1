#!/usr/bin/env python3
"""What keeping world tracks fed by persons one camera sees costs: the three launches follow_rig_poses_in_frames adds
(metro_person_steps_labels, metro_person_rays, metro_associate_tracks_rays), and the whole call next to
follow_world_poses_in_frames on the same boxes.

    python tools/single_view_probe.py [--out FILE] [--quick]   # one JSON object on stdout (and in FILE, default
                                                               # profiles/single_view_probe.json)

16 persons in front of 4 cameras on a ring at 2 time steps; at the second step a quarter of the persons (4) is seen by camera 0
alone: 64 + 52 = 116 boxes, RN50 stride 32 h36m (J = 17, synthetic weights), f16.
  * us per launch on rays that meet (tools/match_probe.py's rig, the second step a copy of the first without the 12 boxes):
    the labels launch, the rays launch, and the association with ray rows under both assignment rules next to
    metro_associate_tracks on the same rows (for which the 4 persons have no step); device events around 200 back-to-back
    launches of the C entry after 20 warm-up launches, median of 5 windows.  Every launch starts from the same empty table (a
    launch never writes the state, so the next one finds every slot free again); it is checked that the 4 ray rows continue the
    tracks the first step bore and that all their joints are placed;
  * calls/s of follow_rig_poses_in_frames against follow_world_poses_in_frames on the same 116 boxes.  Three arms INTERLEAVED
    window by window in one process: world, rig, world again.  The two world arms are the same code on the same data: their
    relative difference (`aa_spread`) is the noise margin the rig arm has to be read against.  Host clock around `calls` calls
    (each ends in its own synchronisation), after 3 warm-up windows, median of 5 windows.  With synthetic weights the forward's
    rays do not meet, so few boxes merge in either arm and most persons are single-view; the launch figures above are the ones
    for a scene that does.
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

PERSONS, STEPS, SINGLE = 16, 2, 4


def scene(spec, rng):
    """-> (cameras, boxes, frame index, person, step, coords01, records) of the 116 boxes, step by step."""
    cams, boxes, fi, pi, coords01, q = rig(spec, PERSONS, rng)
    keep = np.concatenate([np.arange(len(boxes)), np.flatnonzero((pi >= SINGLE) | (fi == 0))])
    step = np.concatenate([np.zeros(len(boxes), np.int32), np.ones(len(keep) - len(boxes), np.int32)])
    q = type(q)(*(a[keep] for a in q))
    return cams, boxes[keep], (fi[keep] + len(cams) * step).astype(np.int32), pi[keep] + PERSONS * step, step, coords01[keep], q


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
    a = 0.5 * (med['world'] + med['world_again'])
    out = {k: {'median': round(med[k], 2), 'windows': [round(v, 2) for v in res[k]]} for k in res}
    out['aa_spread'] = round(abs(med['world'] - med['world_again']) / a, 4)
    out['rig_over_world'] = round(med['rig'] / a, 4)
    return out


def launches(spec, dev, rng, windows, iters):
    sk = spec.skeleton
    _, boxes, fi, pi, step, coords01, q = scene(spec, rng)
    n = len(boxes)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_c01, d_places = up(coords01), up(FR.pack_placements(q)).reshape(-1)
    d_cov = up(np.tile(np.float32([4e-5, 4e-5, 1e-3, 0, 0, 0]), (n, sk.n_head, 1)) * rng.uniform(0.5, 4, (n, sk.n_head, 1)).astype(np.float32))
    times = np.arange(STEPS) / 32.0
    cost, _ = MH.view_affinity_steps(d_c01, d_cov, d_places, fi, step, spec, 1, 'covariance', 2.0, CLIP_MM)
    labels, n_found, rows, starts = MH.cluster_views(cost, MAX_COST_MM)
    assert int(n_found.item()) == PERSONS * STEPS, 'the probe scene must cluster into its persons, step by step'
    poses, _, _, cov = MH.triangulate_joints(d_c01, d_cov, d_places, rows, starts, spec, 'covariance', 2.0, True)
    lib, stream, cs = _lib.load(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), spec.to_c(1)
    p = lambda x: C.c_void_p(x.data_ptr())
    i32 = lambda *k: torch.empty(k, dtype=torch.int32, device=dev)
    mirror, d_step, d_times = up(np.asarray(sk.out_mirror, np.int32)), up(step), up(times)
    person_step, step_rows, step_starts, single = i32(n), i32(n), i32(STEPS + 1), i32(n)
    person_times = torch.empty(n, dtype=torch.float64, device=dev)
    out = {'boxes': n, 'persons_per_step': PERSONS, 'steps': STEPS, 'single_view_persons': SINGLE}
    launch = lambda: _lib.check(lib.metro_person_steps_labels(
        p(labels), p(n_found), n, p(d_step), n, p(d_times), STEPS, p(person_step), p(person_times), p(step_rows), p(step_starts),
        p(single), stream), 'metro_person_steps_labels')
    out['person_steps_labels_us'] = launch_us(launch, windows, iters)
    assert step_starts.tolist() == [0, PERSONS, PERSONS * STEPS] and int((single >= 0).sum()) == SINGLE
    rays = torch.empty((n, sk.n_out, 8), dtype=torch.float64, device=dev)
    launch = lambda: _lib.check(lib.metro_person_rays(
        p(d_c01), p(d_cov), p(d_places), n, C.byref(cs), p(mirror), MH.TRI_WEIGHTS['covariance'], p(single), n, 1, p(rays), stream),
        'metro_person_rays')
    out['person_rays_us'] = launch_us(launch, windows, iters)
    assert int(torch.isfinite(rays[..., 0]).all(dim=1).sum()) == SINGLE
    # the association: every launch from the same empty table
    table = FR.new_track_table(64, sk.n_out, dev)
    ws = torch.empty(lib.metro_associate_tracks_workspace_bytes(64, sk.n_out), dtype=torch.uint8, device=dev)
    track_index, track_id, rows_out, starts_out, n_new, n_dropped, n_unplaced = i32(n), i32(n), i32(n), i32(65), i32(1), i32(1), i32(1)
    track_cost, depth = torch.empty(n, device=dev), torch.empty((n, sk.n_out), device=dev)
    w_poses, w_cov = poses.clone(), cov.clone()
    cj = _lib.MetroSpec(n_joints_out=sk.n_out)
    head = lambda a, b: (p(a), p(b), p(person_times), n, p(step_rows), n, p(step_starts), STEPS, C.byref(cj), _lib.METRO_SMOOTH_COVARIANCE,
                         4e6, 1.0, 1.0, 2000.0, 0.0, 300.0, 600.0, (sk.n_out + 1) // 2, 1.0, p(table.state), 64, p(table.ids),
                         p(table.next_id), p(ws), p(track_index), p(track_id), p(track_cost), p(rows_out), p(starts_out), p(n_new),
                         p(n_dropped))
    for rule, name in ((0, 'greedy'), (1, 'optimal')):
        launch = lambda: _lib.check(lib.metro_associate_tracks_rays(*head(w_poses, w_cov), rule, p(single), p(rays), 1000.0, p(depth),
                                                                     p(n_unplaced), stream), 'metro_associate_tracks_rays')
        out[f'associate_tracks_rays_us_{name}'] = launch_us(launch, windows, iters)
        late = single >= 0
        assert int(n_new.item()) == PERSONS and int(n_unplaced.item()) == 0 and (track_index[late] >= 0).all()
        assert torch.isfinite(depth[late]).all() and int(n_dropped.item()) == 0
    # the plain entry on the same rows: the 4 persons have no step there
    plain = MH.person_steps(rows, starts, n_found, step, times)
    launch = lambda: _lib.check(lib.metro_associate_tracks(*head(poses, cov)[:2], p(plain[1]), n, p(plain[2]), n, p(plain[3]),
                                                           *head(poses, cov)[7:], stream), 'metro_associate_tracks')
    out['associate_tracks_us_greedy'] = launch_us(launch, windows, iters)
    assert int(n_new.item()) == PERSONS and int((track_index >= 0).sum()) == PERSONS * STEPS - SINGLE
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'single_view_probe.json'), help='where the JSON object is written')
    ap.add_argument('--quick', action='store_true', help='fewer windows (under a profiler)')
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('single_view_probe: no HIP device (these numbers exist only on the GPU)')
    windows, iters, calls = (1, 20, 2) if opts.quick else (5, 200, 10)
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    spec = ModelSpec(50, 32, 'h36m')
    result = {'device': torch.cuda.get_device_name(dev),
              'scene': f'{PERSONS} persons x {len(ANGLES)} cameras x {STEPS} steps, {SINGLE} persons on camera 0 alone at the second step, '
                       f'J = {spec.skeleton.n_out}; RN50 stride 32 h36m (synthetic weights), f16; 1920x1080 uint8 frames and boxes on the '
                       'device (geometry=device), cameras 1 and 3 distorted'}
    result['launches'] = launches(spec, dev, rng, windows, iters)

    cams, boxes, fi, _, step, _, _ = scene(spec, rng)
    params = synth.make_params(spec.arch, spec.n_head_channels, spec.base_width, seed=0, logit_gain=synth.logit_gain_for(50, 32))
    frames = [torch.from_numpy(rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8)).to(dev) for _ in range(len(cams) * STEPS)]
    d_boxes = torch.from_numpy(boxes).to(dev)
    stamps = np.repeat(np.arange(STEPS) / 32.0, len(cams))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'rn50_s32.npz')
        save_model(path, spec, params)
        world = lambda: FR.follow_world_poses_in_frames(frames, d_boxes, path, cams * STEPS, fi, stamps, precision='f16')
        rig_call = lambda: FR.follow_rig_poses_in_frames(frames, d_boxes, path, cams * STEPS, fi, stamps, precision='f16')
        result['calls_per_s'] = interleaved_calls_per_s((('world', world), ('rig', rig_call), ('world_again', world)), windows, calls)
        last = rig_call()
        result['synthetic_forward'] = {'persons': int(last.world.poses.shape[0]), 'single_view': int(last.single_view.sum()),
                                       'unplaced': int(last.n_unplaced)}
    text = json.dumps(result, indent=1, sort_keys=True)
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, 'w') as f:
        f.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
