"""metro_associate_tracks_optimal, heads.associate_tracks(assignment=...), frames.follow_world_poses_in_frames(assignment=...)
and frames.Follower on the MI355X: the launch against its fp64 restatement (tests/assign_tracks_ref.py) on the cases of
tests/test_assign_tracks.py with the same bounds, the greedy entry untouched by the keyword, the two rules on the trap scene, and
the Follower against the calls it wraps carried by hand.  Every GPU step runs once."""
import ctypes as C

import numpy as np
import pytest
import torch

from metro_pose3d_amd import _lib, frames as FR, heads as MH
from metro_pose3d_amd._lib import check
from tests import assign_tracks_ref as AR
from tests import follow_tracks_ref as FT

pytestmark = pytest.mark.gpu

CASES, SENTINEL = AR.CASES, FT.SENTINEL


def _up(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _same(a, b):
    """torch.equal with NaN equal to NaN."""
    if not a.is_floating_point():
        return torch.equal(a, b)
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(nan=0.0), b.nan_to_num(nan=0.0))


def _same_tree(a, b, path='result'):
    """Two results of the follow calls, field by field; tensors compared with _same."""
    if isinstance(a, torch.Tensor):
        assert isinstance(b, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype and _same(a, b), path
    elif isinstance(a, tuple):
        assert type(a) is type(b) and len(a) == len(b), path
        for k, (x, y) in enumerate(zip(a, b)):
            _same_tree(x, y, f'{path}.{a._fields[k] if hasattr(a, "_fields") else k}')
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), path
    else:
        assert a == b or a is b, path


def _launch(c, cuda):
    """One metro_associate_tracks_optimal call into outputs pre-filled with the sentinel -> (the dict the comparison reads, the
    device tensors the smoothing launch needs)."""
    n, nj = c['poses'].shape[:2]
    cap = len(c['ids'])
    lib = _lib.load()
    poses, times = _up(np.asarray(c['poses'], np.float32), cuda), _up(np.asarray(c['times'], np.float64), cuda)
    cov = None if c['cov'] is None else _up(np.asarray(c['cov'], np.float32), cuda)
    step_rows, step_starts = _up(np.asarray(c['step_rows'], np.int32), cuda), _up(np.asarray(c['step_starts'], np.int32), cuda)
    state, ids, next_id = _up(np.asarray(c['state'], np.float64), cuda), _up(np.asarray(c['ids'], np.int32), cuda), _up(np.asarray(c['next_id'], np.int32).reshape(1), cuda)
    ints = lambda k: torch.full((k,), SENTINEL, dtype=torch.int32, device=cuda)
    track_index, track_id, rows, starts, n_new, n_dropped = ints(n), ints(n), ints(n), ints(cap + 1), ints(1), ints(1)
    cost = torch.full((n,), float(SENTINEL), dtype=torch.float32, device=cuda)
    ws = torch.full((cap, nj, 28), float(SENTINEL), dtype=torch.float64, device=cuda)
    cs = _lib.MetroSpec(n_joints_out=nj)
    ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    check(lib.metro_associate_tracks_optimal(ptr(poses), ptr(cov), ptr(times), n, ptr(step_rows), len(c['step_rows']), ptr(step_starts),
                                             len(c['step_starts']) - 1, C.byref(cs), MH.SMOOTH_MEASUREMENTS[c['measurement']], c['q'],
                                             c['r_floor'], c['cov_scale'], c['v0'], c['gate'], c['max_cost'], c['clip'], c['min_joints'],
                                             c['max_age'], ptr(state), cap, ptr(ids), ptr(next_id), ptr(ws), ptr(track_index),
                                             ptr(track_id), ptr(cost), ptr(rows), ptr(starts), ptr(n_new), ptr(n_dropped),
                                             C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)), 'metro_associate_tracks_optimal')
    dev = dict(poses=poses, cov=cov, times=times, rows=rows, starts=starts, state=state, working=ws)
    host = lambda t: t.cpu().numpy()
    return dict(track_index=host(track_index), track_id=host(track_id), cost=host(cost), rows=host(rows), starts=host(starts),
                n_new=host(n_new), n_dropped=host(n_dropped), state=host(state), ids=host(ids), next_id=int(next_id.item()),
                working=host(ws)), dev


@pytest.mark.parametrize('name', list(CASES))
def test_kernel_matches_the_restatement_and_the_smoothing_launch(cuda, name):
    """Slots, ids, the CSR, the counts, the table, every t_last and the NaN patterns equal the restatement's, costs within
    1e-3 mm, x and P of the working state within 1e-9 (the bounds of the host-compiled test; every case keeps its optimum
    max(1e-2, 2 min(T, m) 1e-3) mm from the second-best assignment, tests/test_assign_tracks.py); every output written over its
    sentinel.  Live slots 1, 2, 64, 65, 128 against 1, 2, 63, 64, 65, 128 boxes, J = 1, 17, 64, 1, 2 and 65 steps.  A case of
    exact ties is held to the properties every optimum shares.  Then the working state equals, bit for bit, the state
    metro_smooth_tracks (filter mode) writes on the CSR the launch produced."""
    c, want = AR.case_and_expected(name)
    got, dev = _launch(c, cuda)
    worst = AR.compare(got, want, c)
    print(f'{name}: worst cost {worst[0]:.2e} mm, worst state {worst[1]:.2e} rel vs the fp64 restatement')
    for k in ('track_index', 'track_id', 'rows', 'starts', 'n_new', 'n_dropped'):
        assert not (got[k] == SENTINEL).any(), k
    assert not (got['cost'] == SENTINEL).any()
    state = dev['state'].clone()
    MH.smooth_tracks(dev['poses'], dev['cov'], dev['times'], dev['rows'], dev['starts'], 'filter', c['measurement'], c['q'], c['r_floor'],
                     c['cov_scale'], c['v0'], None, state)
    assert _same(state, dev['working']), 'the smoothing launch leaves the working state, bit for bit'
    if c['tie']:
        again, _ = _launch(c, cuda)
        for k in ('track_index', 'track_id', 'cost', 'rows', 'starts', 'ids', 'working'):
            assert np.array_equal(got[k], again[k], equal_nan=True), k


def _associate(c, cuda, lo=0, hi=None, table=None, **kw):
    starts = c['step_starts']
    hi = len(starts) - 1 if hi is None else hi
    table = FR.TrackTable(_up(c['state'], cuda), _up(c['ids'], cuda), _up(np.asarray(c['next_id'], np.int32).reshape(1), cuda)) if table is None else table
    found = MH.associate_tracks(_up(c['poses'], cuda), None if c['cov'] is None else _up(c['cov'], cuda), c['times'],
                                c['step_rows'][starts[lo]:starts[hi]], starts[lo:hi + 1] - starts[lo], *table, **kw)
    return found, table


def test_two_rules_on_the_trap_scene_and_the_default_is_greedy(cuda):
    c = AR.case_and_expected('trap')[0]
    plain, plain_table = _associate(c, cuda)
    greedy, greedy_table = _associate(c, cuda, assignment='greedy')
    for a, b in zip(tuple(plain) + tuple(plain_table), tuple(greedy) + tuple(greedy_table)):
        assert _same(a, b), "assignment='greedy' is the call without the keyword"
    optimal, _ = _associate(c, cuda, assignment='optimal')
    assert greedy.track_id.tolist() == [0, 0, 2, 1, 1, 0] and greedy.n_new.item() == 3
    assert optimal.track_id.tolist() == [0, 0, 0, 1, 1, 1] and optimal.n_new.item() == 2
    assert abs(optimal.cost[2].item() - 120.0) < 1e-3 and abs(optimal.cost[5].item() - 130.0) < 1e-3


def test_stream_cut_into_calls_gives_the_ids_and_states_of_one_call(cuda):
    c, want = AR.case_and_expected('stream')
    nj = c['poses'].shape[1]
    poses, cov = _up(c['poses'], cuda), _up(c['cov'], cuda)

    def run(per_call):
        table = FR.new_track_table(8, nj, cuda)
        ids = torch.full((len(c['poses']),), -1, dtype=torch.int32, device=cuda)
        for lo in range(0, 9, per_call):
            found, _ = _associate(c, cuda, lo, min(lo + per_call, 9), table, assignment='optimal')
            MH.smooth_tracks(poses, cov, c['times'], found.rows, found.starts, 'filter', state=table.state)
            ids = torch.where(found.track_id >= 0, found.track_id, ids)
        return ids, table
    whole_ids, whole = run(9)
    assert np.array_equal(whole_ids.cpu().numpy(), want['track_id'])
    for per_call in (1, 3):
        ids, table = run(per_call)
        assert torch.equal(ids, whole_ids) and torch.equal(table.ids, whole.ids) and _same(table.state, whole.state), per_call


# ---- the Follower against the calls it wraps ------------------------------------------------------------------------------------

def _video():
    """3 boxes on each of 4 small frames, the detector's order changing from frame to frame (frames 2 and 3 repeat the orders of
    frames 0 and 1, so both halves take the same root depths), root depths 1 m apart."""
    from metro_pose3d_amd.camera import Camera
    rng = np.random.default_rng(7)
    frames = [rng.integers(0, 256, (240, 320, 3), dtype=np.uint8) for _ in range(4)]
    cam = Camera(np.array([[300.0, 0, 160], [0, 300.0, 120], [0, 0, 1]]))
    base = np.array([[20.0, 40, 70, 150], [120, 50, 80, 140], [220, 45, 75, 150]])
    order = [[0, 1, 2], [2, 0, 1], [0, 1, 2], [2, 0, 1]]
    boxes = np.concatenate([base[o] + 2.0 * f for f, o in enumerate(order)])
    fi = np.concatenate([[f] * 3 for f in range(4)])
    return frames, cam, boxes, fi, 3000.0 + 1000.0 * np.concatenate(order), np.arange(4) / 32.0


@pytest.mark.parametrize('precision', ['f64', 'f16'])
def test_greedy_follower_is_follow_poses_in_frames_carried_by_hand(cuda, tmp_path, precision):
    from tests.test_gpu_placement import _toy_engine_model
    path = _toy_engine_model(tmp_path)[2]
    frames, cam, boxes, fi, depth, stamps = _video()
    follower = FR.Follower(path, cam, assignment='greedy', capacity=16, scale_recovery='true-root-depth', root_depth=depth[:6],
                           precision=precision)
    assert follower.tracks is None and np.array_equal(depth[:6], depth[6:])
    tracks = None
    for lo, hi in ((0, 2), (2, 4)):                         # two consecutive calls of two frames each
        sel = slice(3 * lo, 3 * hi)
        got = follower.follow(frames[lo:hi], boxes[sel], fi[sel] - lo, stamps[lo:hi])
        want = FR.follow_poses_in_frames(frames[lo:hi], boxes[sel], path, cam, fi[sel] - lo, stamps[lo:hi], tracks=tracks, capacity=16,
                                         scale_recovery='true-root-depth', root_depth=depth[sel], precision=precision)
        tracks = want.tracks
        _same_tree(got, want)
        assert follower.tracks is got.tracks
    assert (got.cost[got.track_id >= 0] >= 0).any(), 'the second call continued tracks of the first'
    sizes = FR.frame_sizes(frames[:2])
    _same_tree(follower.predict(sizes, [4 / 32.0, 5 / 32.0], expand=1.5),
               FR.predict_boxes_in_frames(follower.tracks, cam, sizes, [4 / 32.0, 5 / 32.0], coords='camera', expand=1.5))
    follower.reset()
    assert follower.tracks is None


def test_optimal_follower_is_the_composition_of_its_launches(cuda, tmp_path):
    from tests.test_gpu_placement import _toy_engine_model
    path = _toy_engine_model(tmp_path)[2]
    frames, cam, boxes, fi, depth, stamps = _video()
    follower = FR.Follower(path, cam, assignment='optimal', capacity=16, max_cost_mm=590.0, scale_recovery='true-root-depth',
                           root_depth=depth, precision='f64', mode='filter')
    got = follower.follow(frames, boxes, fi, stamps)
    raw = FR.locate_poses_in_frames(frames, boxes, path, cameras=cam, frame_index=fi, scale_recovery='true-root-depth', root_depth=depth,
                                    precision='f64', return_uncertainty=True)
    table = FR.new_track_table(16, raw.poses.shape[1], cuda)
    times = stamps[fi]
    step_rows, step_starts = FR.time_steps(times)
    with torch.cuda.device(cuda):
        found = MH.associate_tracks(raw.poses, raw.covariance, times, step_rows, step_starts, *table, max_cost_mm=590.0, assignment='optimal')
        smooth = MH.smooth_tracks(raw.poses, raw.covariance, times, found.rows, found.starts, 'filter', state=table.state)
    for a, b in zip((found.track_index, found.track_id, found.cost, found.n_new, found.n_dropped), got[:5]):
        assert _same(a, b)
    _same_tree(tuple(table), tuple(got.tracks))
    for a, b in zip(smooth, got.smoothed[:4]):
        assert _same(a, b)
    assert (got.track_id >= 0).all() and got.tracks is follower.tracks


def test_world_follower_is_follow_world_poses_in_frames(cuda, tmp_path):
    from tests.test_gpu_placement import _toy_engine_model
    from tests.test_gpu_world_follow import _rig
    path = _toy_engine_model(tmp_path)[2]
    cams, frames, boxes, fi, stamps = _rig()
    kw = dict(match_max_cost_mm=600.0, max_cost_mm=590.0, precision='f64')
    follower = FR.Follower(path, cams[:3], world=True, assignment='optimal', capacity=8, **kw)
    tracks = None
    for t in (0, 1):                                        # one exposure of the rig per call
        sel = fi // 3 == t
        got = follower.follow(frames[3 * t:3 * t + 3], boxes[sel], fi[sel] - 3 * t, stamps[3 * t:3 * t + 3])
        want = FR.follow_world_poses_in_frames(frames[3 * t:3 * t + 3], boxes[sel], path, cams[:3], fi[sel] - 3 * t, stamps[3 * t:3 * t + 3],
                                               tracks=tracks, capacity=8, assignment='optimal', **kw)
        tracks = want.tracks
        _same_tree(got, want)
    assert (got.track_id >= 0).any()
    whole = FR.follow_world_poses_in_frames(frames, boxes, path, cams, fi, stamps, capacity=8, assignment='optimal', **kw)
    assert _same(whole.tracks.state, follower.tracks.state) and torch.equal(whole.tracks.ids, follower.tracks.ids)
    sizes = FR.frame_sizes(frames[:3])
    _same_tree(follower.predict(sizes, [0.25] * 3), FR.predict_boxes_in_frames(follower.tracks, cams[:3], sizes, [0.25] * 3, coords='world'))
