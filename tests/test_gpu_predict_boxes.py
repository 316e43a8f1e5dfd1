"""metro_predict_boxes, heads.predict_boxes and frames.predict_boxes_in_frames on the MI355X: the two launches against their fp64
restatement (tests/predict_boxes_ref.py) on the cases of tests/test_predict_boxes.py -- the known answers and the smallest shapes
at each loop boundary of the per-(frame, slot) kernel and of the one-workgroup compaction -- the table left bit for bit as it
was, and the whole chain: the boxes predicted from a follow_* call's table go into the next follow_* call as the CUDA tensors
they are and give what host copies of them give.  Every GPU step runs once."""
import numpy as np
import pytest
import torch

from metro_pose3d_amd import frames as FR, heads as MH
from tests import predict_boxes_ref as PB

pytestmark = pytest.mark.gpu

CASES = PB.CASES


def _up(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _same(a, b):
    """torch.equal with NaN equal to NaN."""
    if not a.is_floating_point():
        return torch.equal(a, b)
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(nan=0.0), b.nan_to_num(nan=0.0))


def _launch(c, cuda):
    """heads.predict_boxes on a case -> (the dict PB.compare reads, the table's tensors before and after)."""
    p = PB.params_of(c)
    state, ids = _up(np.asarray(c['state'], np.float64), cuda), _up(np.asarray(c['ids'], np.int32), cuda)
    before = (state.clone(), ids.clone())
    det = c.get('det_boxes')
    rows = MH.predict_boxes(state, ids, FR.pack_frame_cameras(c['cameras']), np.asarray(c['sizes']), c['times'], c['coords'],
                            None if det is None else _up(np.asarray(det, np.float64), cuda),
                            None if det is None else _up(np.asarray(c['det_frame'], np.int32), cuda), p['expand'], p['n_sigma'],
                            p['max_sigma'], p['min_joints'], p['max_age'], p['near'], p['min_side'], p['iou_max'], p['q'], p['clip'])
    host = lambda t: t.cpu().numpy()
    counts = host(rows.counts)
    n = int(counts[0])
    assert 0 <= n <= len(rows.boxes)
    got = dict(boxes=host(rows.boxes)[:n], frame=host(rows.frame_index)[:n], slot=host(rows.track_index)[:n], id=host(rows.track_id)[:n],
               detection=host(rows.detection)[:n], n_joints=host(rows.n_joints)[:n], counts=counts, dense_boxes=host(rows.dense_boxes),
               dense_joints=host(rows.dense_joints))
    return got, before, (state, ids)


@pytest.mark.parametrize('name', list(CASES))
def test_launch_matches_the_restatement_and_leaves_the_table_alone(cuda, name):
    """Counts, joint counts, the row order and every integer column exact, box coordinates within 1e-2 px on frames up to 4096 px
    (both sides run the projection in fp32 in one order; some ten roundings of at most 2.4e-4 px stay far below); every decision of
    the case at least 1e-1 px (1e-1 mm, 1e-3 of the lens polynomial, 0.01 of IoU, 1e-3 s) from flipping.  The shapes: F T = 1,
    63, 64, 65, 255, 256, 258 (257 is prime and beyond T <= 128, F <= 64), 513; T = 1, 128; F = 1, 64; J = 1, 17, 64; m = 0, 1,
    255, 257; all rows present, none present.  The table is bit for bit what it was."""
    c, want = PB.case_and_expected(name)
    PB.check_margins(c, want)
    got, before, after = _launch(c, cuda)
    worst = PB.compare(got, want)
    print(f'{name}: worst box deviation {worst:.2e} px vs the fp64 restatement')
    assert _same(after[0], before[0]) and torch.equal(after[1], before[1]), 'the table is read, never written'


def _copy(table):
    return FR.TrackTable(*(t.clone() for t in table))


def _rows_on_the_host(pred):
    return pred.boxes.cpu().numpy(), pred.frame_index.cpu().numpy()


@pytest.mark.parametrize('precision', ['f16', 'f64'])
def test_predicted_boxes_go_into_the_next_follow_call_as_they_are(cuda, tmp_path, precision):
    """One camera: follow_poses_in_frames on two frames with host boxes, predict_boxes_in_frames on its table for a third frame,
    and the returned CUDA tensors into follow_poses_in_frames: torch.equal to the same call on host copies of those boxes with
    geometry='device'.  A synthetic model's poses mean nothing: this checks plumbing and equivalence."""
    from metro_pose3d_amd.camera import Camera
    from tests.test_gpu_placement import _toy_engine_model
    spec, _, path = _toy_engine_model(tmp_path)
    rng = np.random.default_rng(7)
    frames = [rng.integers(0, 256, (240, 320, 3), dtype=np.uint8) for _ in range(3)]
    cam = Camera(np.array([[300.0, 0, 160], [0, 300.0, 120], [0, 0, 1]]))
    base = np.array([[20.0, 40, 70, 150], [120, 50, 80, 140], [220, 45, 75, 150]])
    boxes = np.concatenate([base, base[[2, 0, 1]] + 2.0])
    fi, stamps = np.repeat([0, 1], 3), np.arange(3) / 32.0
    depth = 3000.0 + 1000.0 * np.array([0, 1, 2, 2, 0, 1])
    kw = dict(scale_recovery='true-root-depth', precision=precision)
    first = FR.follow_poses_in_frames(frames[:2], boxes, path, cam, fi, stamps[:2], capacity=8, root_depth=depth, **kw)
    table = first.tracks
    kept = _copy(table)
    pred = FR.predict_boxes_in_frames(table, cam, FR.frame_sizes(frames[2:]), stamps[2:], max_sigma_mm=100.0)
    assert all(_same(a, b) for a, b in zip(table, kept)), 'the table is read, never written'
    n = len(pred.boxes)
    print(f'{precision}: {n} predicted boxes for 3 tracks, joints {pred.n_joints.tolist()}, boxes {pred.boxes.round().tolist()}')
    assert n >= 1 and pred.n_predicted == n and pred.boxes.is_cuda and pred.frame_index.is_cuda and pred.boxes.dtype == torch.float64
    assert torch.equal(pred.track_id, table.ids[pred.track_index.long()]) and (pred.detection == -1).all()
    assert pred.dense_boxes.shape == (1, 8, 4) and pred.dense_joints.shape == (1, 8)
    root = 3000.0 + 1000.0 * np.arange(n)
    on_device = FR.follow_poses_in_frames(frames[2:], pred.boxes, path, cam, pred.frame_index, stamps[2:], tracks=_copy(table),
                                          root_depth=root, **kw)
    host_boxes, host_fi = _rows_on_the_host(pred)
    on_host = FR.follow_poses_in_frames(frames[2:], host_boxes, path, cam, host_fi, stamps[2:], tracks=_copy(table), root_depth=root,
                                        geometry='device', **kw)
    for name in ('track_index', 'track_id', 'cost'):
        assert _same(getattr(on_device, name), getattr(on_host, name)), name
    for name in ('poses', 'velocity', 'covariance', 'used', 'state'):
        assert _same(getattr(on_device.smoothed, name), getattr(on_host.smoothed, name)), name
    assert torch.equal(on_device.tracks.ids, on_host.tracks.ids)
    # a detector's boxes of that frame: the one on a predicted box is left out, the one in a corner is appended
    det = torch.cat([pred.boxes[:1], torch.tensor([[300.0, 2.0, 12.0, 20.0]], dtype=torch.float64, device=cuda)])
    fused = FR.predict_boxes_in_frames(table, cam, FR.frame_sizes(frames[2:]), stamps[2:], detections=det, max_sigma_mm=100.0)
    assert fused.n_predicted == n and fused.n_suppressed == 1 and fused.n_bad_detections == 0
    assert fused.detection.tolist() == [-1] * n + [1] and torch.equal(fused.boxes[n], det[1]) and torch.equal(fused.boxes[:n], pred.boxes)


@pytest.mark.parametrize('precision', ['f16', 'f64'])
def test_predicted_boxes_go_into_the_next_world_follow_call_as_they_are(cuda, tmp_path, precision):
    """A 3-camera rig: follow_world_poses_in_frames on two exposures, predict_boxes_in_frames(coords='world') on its table for a
    third, and the returned CUDA tensors into follow_world_poses_in_frames: torch.equal to host copies with geometry='device'."""
    from tests.test_gpu_placement import _toy_engine_model
    from tests.test_gpu_world_follow import _rig
    spec, _, path = _toy_engine_model(tmp_path)
    cams, frames, boxes, fi, stamps = _rig()
    kw = dict(match_max_cost_mm=600.0, max_cost_mm=590.0, precision=precision)
    first = FR.follow_world_poses_in_frames(frames, boxes, path, cams, fi, stamps, capacity=8, **kw)
    table = first.tracks
    assert (table.ids >= 0).any()
    kept = _copy(table)
    nxt = [0.25] * 3
    pred = FR.predict_boxes_in_frames(table, cams[:3], FR.frame_sizes(frames[:3]), nxt, coords='world', max_sigma_mm=100.0)
    assert all(_same(a, b) for a, b in zip(table, kept)), 'the table is read, never written'
    n = len(pred.boxes)
    print(f'{precision}: {n} predicted boxes on 3 cameras for ids {table.ids[table.ids >= 0].tolist()}: frames {pred.frame_index.tolist()}, '
          f'slots {pred.track_index.tolist()}, joints {pred.n_joints.tolist()}')
    assert n >= 2 and pred.boxes.is_cuda and (pred.frame_index[1:] >= pred.frame_index[:-1]).all(), 'frame-major'
    on_device = FR.follow_world_poses_in_frames(frames[:3], pred.boxes, path, cams[:3], pred.frame_index, nxt, tracks=_copy(table), **kw)
    host_boxes, host_fi = _rows_on_the_host(pred)
    on_host = FR.follow_world_poses_in_frames(frames[:3], host_boxes, path, cams[:3], host_fi, nxt, tracks=_copy(table), geometry='device',
                                              **kw)
    for name in ('person_index', 'cost', 'track_index', 'track_id', 'track_cost'):
        assert _same(getattr(on_device, name), getattr(on_host, name)), name
    assert _same(on_device.world.poses, on_host.world.poses)
    for name in ('poses', 'velocity', 'covariance', 'used', 'state'):
        assert _same(getattr(on_device.smoothed, name), getattr(on_host.smoothed, name)), name


def test_bad_detection_frame_index_raises_after_the_synchronisation(cuda):
    c, _ = PB.case_and_expected('detections')
    table = FR.TrackTable(_up(np.asarray(c['state'], np.float64), cuda), _up(np.asarray(c['ids'], np.int32), cuda),
                          torch.zeros(1, dtype=torch.int32, device=cuda))
    det = _up(np.asarray(c['det_boxes']), cuda)
    good = FR.predict_boxes_in_frames(table, c['cameras'], c['sizes'], c['times'], detections=det, detection_frame_index=c['det_frame'])
    assert (len(good.boxes), good.n_predicted, good.n_suppressed, good.n_bad_detections) == (6, 3, 1, 2)
    for bad in ([0, 0, 0, 2, 0, 0], _up(np.asarray([0, -1, 0, 1, 0, 0], np.int64), cuda)):
        with pytest.raises(ValueError, match=r'frame_index must lie in \[0, 2\)'):
            FR.predict_boxes_in_frames(table, c['cameras'], c['sizes'], c['times'], detections=det, detection_frame_index=bad)
    # no detections and an empty table: rows of none
    empty = FR.predict_boxes_in_frames(FR.new_track_table(4, 17, cuda), c['cameras'], c['sizes'], c['times'])
    assert len(empty.boxes) == 0 and empty.n_predicted == 0 and (empty.dense_joints == -1).all() and torch.isnan(empty.dense_boxes).all()
