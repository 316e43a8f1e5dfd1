"""metro_associate_tracks, heads.associate_tracks and frames.follow_poses_in_frames on the MI355X: the launch against its fp64
restatement (tests/follow_tracks_ref.py) on the cases of tests/test_follow_tracks.py -- the known answers and the smallest
shapes at each loop boundary of the one-workgroup walk -- the working state against the smoothing launch, the table carried
across calls, and the whole call against track_poses_in_frames given the track_index it found.  Every GPU step runs once."""
import ctypes as C

import numpy as np
import pytest
import torch

from metro_pose3d_amd import _lib, frames as FR, heads as MH
from metro_pose3d_amd._lib import check
from tests import follow_tracks_ref as FT

pytestmark = pytest.mark.gpu

CASES, SENTINEL = FT.CASES, FT.SENTINEL


def _up(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _same(a, b):
    """torch.equal with NaN equal to NaN."""
    if not a.is_floating_point():
        return torch.equal(a, b)
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(nan=0.0), b.nan_to_num(nan=0.0))


def _launch(c, cuda):
    """One metro_associate_tracks call into outputs pre-filled with the sentinel -> (the dict FT.compare reads as NumPy arrays,
    the device tensors the smoothing launch needs)."""
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
    assert lib.metro_associate_tracks_workspace_bytes(cap, nj) == cap * nj * 28 * 8
    ws = torch.full((cap, nj, 28), float(SENTINEL), dtype=torch.float64, device=cuda)
    cs = _lib.MetroSpec(n_joints_out=nj)
    ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    check(lib.metro_associate_tracks(ptr(poses), ptr(cov), ptr(times), n, ptr(step_rows), len(c['step_rows']), ptr(step_starts),
                                     len(c['step_starts']) - 1, C.byref(cs), MH.SMOOTH_MEASUREMENTS[c['measurement']], c['q'], c['r_floor'],
                                     c['cov_scale'], c['v0'], c['gate'], c['max_cost'], c['clip'], c['min_joints'], c['max_age'], ptr(state),
                                     cap, ptr(ids), ptr(next_id), ptr(ws), ptr(track_index), ptr(track_id), ptr(cost), ptr(rows),
                                     ptr(starts), ptr(n_new), ptr(n_dropped), C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)),
          'metro_associate_tracks')
    dev = dict(poses=poses, cov=cov, times=times, rows=rows, starts=starts, state=state, working=ws)
    host = lambda t: t.cpu().numpy()
    return dict(track_index=host(track_index), track_id=host(track_id), cost=host(cost), rows=host(rows), starts=host(starts),
                n_new=host(n_new), n_dropped=host(n_dropped), state=host(state), ids=host(ids), next_id=int(next_id.item()),
                working=host(ws)), dev


@pytest.mark.parametrize('name', list(CASES))
def test_kernel_matches_the_restatement_and_the_smoothing_launch(cuda, name):
    """track_index, track_id, the CSR, the counts, the table, every t_last and the NaN patterns equal the restatement's, costs
    within 1e-3 mm, x and P of the working state within 1e-9 (the bounds of the host-compiled test; every case keeps its
    decisions 1e-2 mm from flipping, tests/test_follow_tracks.py); every output written over its sentinel.  The shapes straddle
    the 256 threads and the wave: capacity 1, 2, 65, 128; 1, 64, 65, 128 boxes in a step; J = 1, 17, 64; 1, 2, 65 steps.
    Then the working state equals, bit for bit, the state metro_smooth_tracks (filter mode) writes on the CSR the launch
    produced."""
    c, want = FT.case_and_expected(name)
    got, dev = _launch(c, cuda)
    worst = FT.compare(got, want, c)
    print(f'{name}: worst cost {worst[0]:.2e} mm, worst state {worst[1]:.2e} rel vs the fp64 restatement')
    for k in ('track_index', 'track_id', 'rows', 'starts', 'n_new', 'n_dropped'):
        assert not (got[k] == SENTINEL).any(), k
    assert not (got['cost'] == SENTINEL).any()
    state = dev['state'].clone()
    MH.smooth_tracks(dev['poses'], dev['cov'], dev['times'], dev['rows'], dev['starts'], 'filter', c['measurement'], c['q'], c['r_floor'],
                     c['cov_scale'], c['v0'], None, state)
    assert _same(state, dev['working']), 'the smoothing launch leaves the working state, bit for bit'


def test_table_carried_across_two_calls_gives_the_ids_of_one_call(cuda):
    """heads.associate_tracks + heads.smooth_tracks on the newcomer case cut after frame 3, the table carried: the ids and the
    final state of the single call; track_index, rows and starts stay on the device."""
    c, want = FT.case_and_expected('newcomer')
    poses, cov = _up(c['poses'], cuda), _up(c['cov'], cuda)
    nj, starts = c['poses'].shape[1], c['step_starts']

    def run(table, lo, hi):
        found = MH.associate_tracks(poses, cov, c['times'], c['step_rows'][starts[lo]:starts[hi]], starts[lo:hi + 1] - starts[lo], *table)
        MH.smooth_tracks(poses, cov, c['times'], found.rows, found.starts, 'filter', state=table.state)
        assert found.track_index.device.type == 'cuda' and found.rows.dtype == torch.int32 and _same(found.working_state, table.state)
        return found
    whole_table, table = FR.new_track_table(8, nj, cuda), FR.new_track_table(8, nj, cuda)
    whole = run(whole_table, 0, len(starts) - 1)
    assert np.array_equal(whole.track_id.cpu().numpy(), want['track_id']) and whole_table.next_id.item() == 2
    a = run(table, 0, 4)
    b = run(table, 4, len(starts) - 1)
    first = torch.from_numpy(np.isin(np.arange(len(c['poses'])), c['step_rows'][:starts[4]])).to(cuda)
    assert torch.equal(torch.where(first, a.track_id, b.track_id), whole.track_id)
    assert a.n_new.item() == 2 and b.n_new.item() == 0 and (b.cost[~first & (b.track_id >= 0)] > 0).all()
    assert _same(table.state, whole_table.state) and torch.equal(table.ids, whole_table.ids) and table.next_id.item() == 2


def test_no_boxes_launch_nothing(cuda):
    table = FR.new_track_table(4, 17, cuda)
    before = [t.clone() for t in table]
    found = MH.associate_tracks(torch.zeros((0, 17, 3), device=cuda), torch.zeros((0, 17, 3, 3), device=cuda), [], [], [0], *table)
    assert found.track_index.shape == (0,) and found.starts.tolist() == [0] * 5 and found.n_new.item() == 0 and found.n_dropped.item() == 0
    # boxes but no steps: every box untracked, the table untouched
    found = MH.associate_tracks(torch.zeros((3, 17, 3), device=cuda), None, [0.0, 0.0, 0.1], [], [0], *table, measurement='isotropic')
    assert found.track_index.tolist() == [-1] * 3 and found.rows.tolist() == [-1] * 3 and torch.isnan(found.cost).all()
    for t, b in zip(table, before):
        assert _same(t, b)


@pytest.mark.parametrize('boxes_on', ['host', 'device'])
@pytest.mark.parametrize('precision', ['f64', 'f16'])
@pytest.mark.parametrize('mode', ['filter', 'smooth'])
def test_follow_poses_in_frames_is_track_poses_in_frames_with_the_index_it_found(cuda, tmp_path, mode, precision, boxes_on):
    """3 boxes on each of 3 small frames plus one box on a fourth, root depths 1 m apart so that the persons are: `smoothed` is
    torch.equal to track_poses_in_frames called with the track_index found and a clone of the starting state; a second call
    carries the table."""
    from metro_pose3d_amd.camera import Camera
    from tests.test_gpu_placement import _toy_engine_model
    spec, _, path = _toy_engine_model(tmp_path)
    rng = np.random.default_rng(7)
    frames = [rng.integers(0, 256, (240, 320, 3), dtype=np.uint8) for _ in range(4)]
    cam = Camera(np.array([[300.0, 0, 160], [0, 300.0, 120], [0, 0, 1]]))
    base = np.array([[20.0, 40, 70, 150], [120, 50, 80, 140], [220, 45, 75, 150]])
    order = [[0, 1, 2], [2, 0, 1], [1, 2, 0], [1]]          # the detector's order changes from frame to frame
    boxes = np.concatenate([base[o] + 2.0 * f for f, o in enumerate(order)])
    fi = np.concatenate([[f] * len(o) for f, o in enumerate(order)])
    person = np.concatenate(order)
    depth = 3000.0 + 1000.0 * person
    stamps = np.arange(4) / 32.0
    kw = dict(scale_recovery='true-root-depth', root_depth=depth, precision=precision, mode=mode)
    d_boxes = torch.from_numpy(boxes).to(cuda) if boxes_on == 'device' else boxes
    start = FR.new_track_table(16, spec.skeleton.n_out, cuda)
    start_state = start.state.clone()
    got = FR.follow_poses_in_frames(frames, d_boxes, path, cam, fi, stamps, tracks=start, **kw)
    assert got.track_index.device.type == 'cuda' and got.tracks.state is start.state and got.smoothed.state is start.state
    ti = got.track_index.cpu().numpy()
    assert (ti >= 0).all() and got.n_dropped.item() == 0, 'every box is tracked'
    want = FR.track_poses_in_frames(frames, d_boxes, path, cam, ti, fi, stamps, state=start_state, **kw)
    for name in ('poses', 'velocity', 'covariance', 'used', 'state'):
        assert _same(getattr(got.smoothed, name), getattr(want, name)), name
    assert torch.equal(got.smoothed.raw.poses, want.raw.poses)
    by_person = {p: set(got.track_id.cpu().numpy()[person == p].tolist()) for p in range(3)}
    print(f'{mode}, {precision}, {boxes_on} boxes: ids per person {by_person}, new {got.n_new.item()}')
    assert got.n_new.item() == len(set(got.track_id.tolist())) and got.tracks.next_id.item() == got.n_new.item()
    nxt = FR.follow_poses_in_frames(frames[:1], d_boxes[:3], path, cam, fi[:3], [4 / 32.0], tracks=got.tracks, **{**kw, 'root_depth': depth[:3]})
    assert nxt.tracks.state is start.state and (nxt.tracks.state[nxt.track_index.long(), :, 27] == 4 / 32.0).all()
