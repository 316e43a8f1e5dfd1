"""Next-frame person boxes from the track table, without a GPU: the fp64 restatement the GPU tests compare against
(tests/predict_boxes_ref.py) on known answers, the closed loop with the smoothing restatement (a filtered walker is boxed where it
will be), the kernel's own code compiled for the host against that restatement on every case and at every loop boundary, the
margin that keeps every case away from a decision the tolerance could flip, the argument checks of the Python surface that run
before any device is touched, and the new C symbol in header, bindings and library with its invalid-argument returns.

F T = 257 is prime and lies beyond both limits (T <= 128, F <= 64), so no table has that many rows: the cases take 258 = 6 x 43,
the smallest size past the compaction's 256-row chunk that a table can have."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from metro_pose3d_amd import _lib, frames as FR, heads as MH
from metro_pose3d_amd.camera import Camera
from tests import predict_boxes_ref as PB
from tests import track_smoothing_ref as TS
from tests.helpers import compile_for_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = PB.CASES


def _true_pixels(cam, points, coords='camera'):
    """fp64 pinhole / lens model of camera points, written out: the pixels a joint at `points` has."""
    p = np.asarray(points, np.float64)
    if coords == 'world':
        p = (p - cam.t.astype(np.float64)) @ cam.R.astype(np.float64).T
    xy = p[:, :2] / p[:, 2:]
    if cam.distortion_coeffs is not None:
        k1, k2, p1, p2, k3 = (float(v) for v in cam.distortion_coeffs)
        r2 = (xy ** 2).sum(axis=1)
        radial = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3 + 2 * p2 * xy[:, 0] + 2 * p1 * xy[:, 1]
        xy = np.stack([xy[:, 0] * radial + p2 * r2, xy[:, 1] * radial + p1 * r2], axis=1)
    k = cam.intrinsic_matrix.astype(np.float64)
    return xy @ k[:2, :2].T + k[:2, 2]


def _bbox(uv):
    lo, hi = uv.min(axis=0), uv.max(axis=0)
    return np.array([lo[0], lo[1], hi[0] - lo[0], hi[1] - lo[1]])


def _about_centre(box, factor):
    c = box[:2] + box[2:] / 2
    return np.concatenate([c - box[2:] / 2 * factor, box[2:] * factor])


def _joints_at(c, slot, t):
    """The constant-velocity positions [J, 3] of a slot's joints at time t."""
    s = c['state'][slot]
    return s[:, :3] + (t - s[:, 27:28]) * s[:, 3:6]


# ---- the restatement on known answers ------------------------------------------------------------------------------------------

def test_standing_person_gets_the_bounding_box_of_its_joints_times_expand():
    c, r = PB.case_and_expected('tight')
    uv = _true_pixels(c['cameras'][0], _joints_at(c, 1, 0.1))
    assert r['counts'].tolist() == [1, 1, 0, 0, 0] and (r['slot'], r['id'], r['frame'], r['n_joints']) == ([1], [5], [0], [17])
    assert np.abs(r['boxes'][0] - _bbox(uv)).max() < 1e-3, 'expand = 1, n_sigma = 0: the bounding box of the projections'
    grown = PB.predict(dict(c, params=dict(expand=1.25, n_sigma=0.0)))
    assert np.abs(grown['boxes'][0] - _about_centre(_bbox(uv), 1.25)).max() < 1e-3
    # the body spans 500 x 1700 mm at about 4 m under f = 1000: about 125 x 425 px
    assert 120 < r['boxes'][0, 2] < 135 and 410 < r['boxes'][0, 3] < 450
    c, r = PB.case_and_expected('standing')
    assert (r['boxes'][0, 2:] > grown['boxes'][0, 2:]).all(), 'the defaults add the margin of the predicted covariance'


def test_velocity_moves_the_box_by_f_v_dt_over_z():
    flat = PB.body(17) * [1, 1, 0] + [0, 0, 4000.0]
    boxes = []
    for v in (0.0, 1200.0):
        state, ids = PB.table(1, 17)
        PB.put(state, ids, 0, 0, flat, velocity=(v, 0, 0))
        boxes.append(PB.predict(dict(state=state, ids=ids, cameras=[PB.pinhole()], sizes=[[1280, 720]], times=[0.1], coords='camera',
                                     params=dict(expand=1.0, n_sigma=0.0)))['boxes'][0])
    assert np.abs(boxes[1] - boxes[0] - [1000.0 * 1200.0 * 0.1 / 4000.0, 0, 0, 0]).max() < 1e-3


def test_margin_grows_with_dt_and_stops_at_max_sigma():
    c, r = PB.case_and_expected('growth')
    w = r['dense_boxes'][:, 0, 2]
    assert (np.diff(w[:6]) > 0.5).all(), 'dt 0 to 0.8 s: the position variance grows'
    assert np.abs(np.diff(w[5:])).max() < 1e-9, 'sigma has reached max_sigma_mm: 0.8, 0.9 and 0.95 s give one box'
    bare = PB.predict(dict(c, params=dict(expand=1.0, clip=False, n_sigma=0.0)))['dense_boxes'][:, 0, 2]
    # the widest joint margin on either side: n_sigma * 300 mm * f / z of the outermost joints (z within 100 mm of 5000)
    assert np.abs((w[5:] - bare[5:]) / 2 - 2.0 * 300.0 * 1000.0 / 5000.0).max() < 3.0


def test_slots_without_a_box():
    c, r = PB.case_and_expected('no-box')
    assert r['dense_joints'][0].tolist() == [-1, -1, 0, 5, 17, 17, -1, 17]
    assert np.flatnonzero(~np.isnan(r['dense_boxes'][0, :, 0])).tolist() == [5, 7] and r['slot'].tolist() == [5, 7]
    across = r['boxes'][0]
    unclipped = PB.predict(dict(c, params=dict(clip=False)))
    assert unclipped['slot'].tolist() == [4, 5, 7], 'without clip the person left of the frame has a box'
    assert unclipped['boxes'][0, 0] + unclipped['boxes'][0, 2] < 0, 'wholly outside the frame'
    wide = unclipped['boxes'][1]
    assert wide[0] < 0 and across[0] == 0.0 and abs(across[0] + across[2] - (wide[0] + wide[2])) < 1e-9, 'clipped at the left border'
    assert np.array_equal(r['boxes'][1], unclipped['boxes'][2])


def test_joint_beyond_the_monotonic_range_is_skipped():
    c, r = PB.case_and_expected('fold')
    cam = c['cameras'][0]
    folded = PB.pixels(cam, c['state'][0, 1:2, :3])[0]
    assert 0 < folded[0] < 1280 and 0 < folded[1] < 720, 'the polynomial folds the far joint back into the image'
    assert r['n_joints'].tolist() == [3]
    assert r['boxes'][0, 0] + r['boxes'][0, 2] < folded[0] - 100, 'and the box does not reach for it'
    assert np.abs(r['boxes'][0] - _bbox(_true_pixels(cam, c['state'][0, [0, 2, 3], :3]))).max() < 1e-3


def test_world_coordinates_give_one_box_per_camera_around_the_true_projections():
    c, r = PB.case_and_expected('world-rig')
    assert r['frame'].tolist() == [0, 1, 2] and r['slot'].tolist() == [1, 1, 1] and r['id'].tolist() == [3, 3, 3]
    for f, cam in enumerate(c['cameras']):
        uv = _true_pixels(cam, _joints_at(c, 1, 0.1), 'world')
        b = r['boxes'][f]
        assert (uv >= b[:2]).all() and (uv <= b[:2] + b[2:]).all()
    assert len({tuple(np.round(b)) for b in r['boxes']}) == 3, 'three cameras, three different boxes'


def test_camera_coordinates_ignore_r_and_t():
    c, r = PB.case_and_expected('camera-ignores-rt')
    plain = [Camera(cam.intrinsic_matrix, cam.distortion_coeffs) for cam in c['cameras']]
    assert np.array_equal(PB.predict(dict(c, cameras=plain))['boxes'], r['boxes']) and len(r['boxes']) == 3


def test_detections_are_fused_in_their_order():
    c, r = PB.case_and_expected('detections')
    assert r['counts'].tolist() == [6, 3, 1, 2, 0]
    assert r['frame'].tolist() == [0, 0, 1, 0, 1, 0] and r['slot'].tolist() == [0, 2, 0, -1, -1, -1]
    assert r['id'].tolist() == [7, 9, 7, -1, -1, -1] and r['detection'].tolist() == [-1, -1, -1, 0, 3, 5]
    assert r['n_joints'].tolist() == [17, 17, 17, -1, -1, -1]
    assert np.array_equal(r['boxes'][3:], c['det_boxes'][[0, 3, 5]])
    person = PB._corners(r['dense_boxes'][0, 0])
    above, below = PB.overlap(PB._corners(c['det_boxes'][2]), person), PB.overlap(PB._corners(c['det_boxes'][0]), person)
    assert 0.3 < above < 0.35 and 0.25 < below < 0.3, 'one on either side of iou_max'
    assert PB.overlap(PB._corners(c['det_boxes'][3]), PB._corners(r['dense_boxes'][0, 2])) == 1.0, 'kept: that box is on another frame'
    c, r = PB.case_and_expected('bad-frames')
    assert r['counts'].tolist() == [5, 3, 1, 1, 2] and r['detection'].tolist() == [-1, -1, -1, 0, 5], 'the frame is looked at first'


# ---- the closed loop with the smoothing restatement ---------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def walker():
    """A person walking at 1.5 m/s across a distorted camera at 4.5 m, 30 fps, 10 frames measured exactly and filtered by the
    smoothing restatement; its state is the table."""
    nj, fps = 17, 30.0
    start, vel = PB.body(nj) + [-600.0, 0, 4500.0], np.array([1500.0, 0, 0])
    at = lambda t: start + t * vel
    times = np.arange(10) / fps
    poses = np.stack([at(t) for t in times])
    state = np.full((1, nj, 28), np.nan)
    *_, state = TS.smooth_tracks(poses, None, times, np.arange(10), [0, 10], 'filter', 'isotropic', state=state)
    assert np.abs(state[0, :, :3] - at(times[-1])).max() < 5e-12 * 1e3 and np.abs(state[0, :, 3:6] - vel).max() < 1e-6
    cam = PB.pinhole(distortion_coeffs=PB.DISTORTION)
    return dict(state=state, ids=np.array([4], np.int32), cameras=[cam], sizes=[[1280, 720]] * 2, times=[10 / fps, 14 / fps],
                coords='camera'), at


def test_filtered_walker_is_boxed_where_it_will_be(walker):
    c, at = walker
    r = PB.predict(dict(c, params=dict(expand=1.0, n_sigma=0.0)))
    loose = PB.predict(c)
    assert r['frame'].tolist() == [0, 1] == loose['frame'].tolist()
    for f, t in enumerate(c['times']):
        uv = _true_pixels(c['cameras'][0], at(t))
        dev = np.abs(r['boxes'][f] - _bbox(uv)).max()
        print(f'frame {f} ({t:.3f} s): box vs the true next projections {dev:.2e} px')
        assert dev <= 1e-2
        b = loose['boxes'][f]
        assert (uv >= b[:2]).all() and (uv <= b[:2] + b[2:]).all(), 'the default box contains every true projection'


# ---- the kernel's own code on the host --------------------------------------------------------------------------------------------

def run_on_host(fn, c):
    """One call of the host-compiled kernel code on a case -> the dict PB.compare reads.  Outputs are pre-filled with the sentinel."""
    p = PB.params_of(c)
    state, ids = np.ascontiguousarray(c['state'], np.float64), np.ascontiguousarray(c['ids'], np.int32)
    n_tracks, nj = state.shape[:2]
    sizes, times = np.ascontiguousarray(c['sizes'], np.int32), np.ascontiguousarray(c['times'], np.float64)
    cameras = FR.pack_frame_cameras(c['cameras'])
    n_frames = len(times)
    m = 0 if c.get('det_boxes') is None else len(c['det_boxes'])
    det = np.ascontiguousarray(c['det_boxes'], np.float64) if m else None
    det_frame = np.ascontiguousarray(c['det_frame'], np.int32) if m else None
    cap = n_frames * n_tracks + m
    ints = lambda *shape: np.full(shape, PB.SENTINEL, np.int32)
    outs = [np.full((n_frames, n_tracks, 4), float(PB.SENTINEL)), ints(n_frames, n_tracks), np.full((cap, 4), float(PB.SENTINEL)),
            ints(cap), ints(cap), ints(cap), ints(cap), ints(cap), ints(5)]
    ptr = lambda a: C.c_void_p(a.ctypes.data if a is not None else 0)
    fn(ptr(state), ptr(ids), n_tracks, nj, ptr(cameras), len(cameras), ptr(sizes), ptr(times), n_frames, MH._COORDS[c['coords']], p['q'],
       p['max_age'], p['expand'], p['n_sigma'], p['max_sigma'], p['near'], p['min_side'], p['min_joints'], int(p['clip']), ptr(det),
       ptr(det_frame), m, p['iou_max'], *[ptr(o) for o in outs])
    dense, dense_joints, boxes, frame, slot, tid, detection, joints, counts = outs
    n = int(counts[0])
    assert 0 <= n <= cap
    for a in (boxes, frame, slot, tid, detection, joints):
        assert (a[n:] == PB.SENTINEL).all(), 'rows past counts[0] are not written'
    for a in (frame[:n], slot[:n], detection[:n], dense_joints):
        assert not (a == PB.SENTINEL).any()
    return dict(boxes=boxes[:n], frame=frame[:n], slot=slot[:n], id=tid[:n], detection=detection[:n], n_joints=joints[:n], counts=counts,
                dense_boxes=dense, dense_joints=dense_joints)


@pytest.fixture(scope='module')
def host_kernel(tmp_path_factory):
    """predict_boxes.hip's steps are __host__ __device__ functions of one index: the source compiled for the host and run by one
    thread in the kernels' order, a running count where the workgroup has its ballots and per-wave sums."""
    tmp = tmp_path_factory.mktemp('host_predict_boxes')
    fn = compile_for_host(tmp, 'host_predict_boxes', ['predict_boxes.hip'], '''
extern "C" void host_predict_boxes(const double* state, const int* ids, int n_tracks, int n_out, const MetroFrameCamera* cameras,
                                   int n_cameras, const int* frame_sizes, const double* frame_times, int n_frames, int coords, double q,
                                   double max_age, double expand, double n_sigma, double max_sigma, double near, double min_side,
                                   int min_joints, int clip, const double* det_boxes, const int* det_frame, int n_det, double iou_max,
                                   double* boxes_dense, int* joints_dense, double* boxes_out, int* frame_out, int* slot_out, int* id_out,
                                   int* detection_out, int* n_joints_out, int* counts) {
    using namespace metro;
    const PredictArgs a = make_predict_args(state, ids, n_tracks, n_out, cameras, n_cameras, frame_sizes, frame_times, n_frames, coords,
                                            q, max_age, expand, n_sigma, max_sigma, near, min_side, min_joints, clip, det_boxes,
                                            det_frame, n_det, iou_max, boxes_dense, joints_dense, boxes_out, frame_out, slot_out,
                                            id_out, detection_out, n_joints_out, counts);
    for (int idx = 0; idx < n_frames * n_tracks; ++idx) predict_one(a, idx);
    int at = 0, tally[4] = {0, 0, 0, 0};
    for (int idx = 0; idx < n_frames * n_tracks; ++idx)
        if (compact_present(a, idx)) compact_write_predicted(a, idx, at++);
    const int n_predicted = at;
    for (int k = 0; k < n_det; ++k) {
        const int verdict = compact_detection(a, k);
        ++tally[verdict];
        if (verdict == DET_KEPT) compact_write_detection(a, k, at++);
    }
    counts[0] = at; counts[1] = n_predicted;
    counts[2] = tally[DET_SUPPRESSED]; counts[3] = tally[DET_BAD]; counts[4] = tally[DET_BAD_FRAME];
}
''').host_predict_boxes
    fn.restype = None
    fn.argtypes = _lib.SIGNATURES['metro_predict_boxes'][1][:-1]

    return lambda c: run_on_host(fn, c)


@pytest.mark.parametrize('name', list(CASES))
def test_kernel_code_on_the_host_matches_the_restatement(host_kernel, name):
    """Counts, joint counts, the row order and every integer column exact; box coordinates within 1e-2 px on frames up to 4096 px:
    both sides run the projection in fp32 in one order, and some ten roundings of at most half an fp32 ulp at 4096 (2.4e-4 px)
    stay far below the bound.  Every decision of the case is at least 1e-1 px (1e-1 mm of depth, 1e-3 of the lens polynomial,
    0.01 of IoU, 1e-3 s of age) from flipping, so the tolerance cannot change one."""
    c, want = PB.case_and_expected(name)
    PB.check_margins(c, want)
    worst = PB.compare(host_kernel(c), want)
    print(f"{name}: worst box deviation {worst:.2e} px vs the fp64 restatement; margins {want['margins']}")


def test_cases_cover_every_loop_boundary():
    shapes = {name: (len(c['times']), *c['state'].shape[:2], 0 if c.get('det_boxes') is None else len(c['det_boxes']))
              for name, c in ((name, PB.case_and_expected(name)[0]) for name in CASES)}
    rows = {f * t for f, t, _, _ in shapes.values()}
    assert {1, 63, 64, 65, 255, 256, 258, 513} <= rows, '257 is prime and beyond T <= 128, F <= 64: 258 stands in'
    assert {1, 128} <= {t for _, t, _, _ in shapes.values()} and {1, 64} <= {f for f, _, _, _ in shapes.values()}
    assert {1, 17, 64} <= {j for _, _, j, _ in shapes.values()} and {0, 1, 255, 257} <= {m for _, _, _, m in shapes.values()}
    full = PB.case_and_expected('ft513-all')[1]
    assert full['counts'][0] == 513 and not np.isnan(full['dense_boxes']).any(), 'all rows present'
    assert PB.case_and_expected('none-present')[1]['counts'][1] == 0, 'none present'


# ---- the Python surface ---------------------------------------------------------------------------------------------------------

def test_frame_sizes_on_all_pixel_formats():
    u8 = lambda *shape: np.zeros(shape, np.uint8)
    assert FR.frame_sizes([u8(48, 64, 3), torch.zeros((20, 30, 3), dtype=torch.uint8)]).tolist() == [[64, 48], [30, 20]]
    assert FR.frame_sizes(u8(48, 64, 3), 'bgr').tolist() == [[64, 48]]
    assert FR.frame_sizes([u8(72, 64), (u8(20, 30), u8(10, 15, 2)), (u8(20, 30), u8(10, 30))], 'nv12').tolist() == [[64, 48], [30, 20], [30, 20]]
    assert FR.frame_sizes([u8(72, 64), (u8(20, 32), u8(10, 16), u8(10, 16))], 'i420').tolist() == [[64, 48], [32, 20]]
    sizes = FR.frame_sizes(u8(72, 64), 'nv12')
    assert sizes.dtype == np.int32 and sizes.shape == (1, 2)
    with pytest.raises(ValueError, match='pixel_format'):
        FR.frame_sizes(u8(48, 64, 3), 'yuyv')
    with pytest.raises(ValueError, match='rows are not'):
        FR.frame_sizes(u8(70, 64), 'nv12')
    with pytest.raises(ValueError, match='frame 0'):
        FR.frame_sizes(u8(48, 64), 'rgb')


def test_python_surface_checks_arguments_without_a_gpu():
    d = {k: v.default for k, v in inspect.signature(FR.predict_boxes_in_frames).parameters.items()}
    assert list(d) == ['tracks', 'cameras', 'frame_sizes', 'timestamps', 'coords', 'detections', 'detection_frame_index', 'expand',
                       'n_sigma', 'max_sigma_mm', 'min_joints', 'max_age_s', 'near_mm', 'min_side_px', 'iou_max', 'accel_psd', 'clip']
    assert [d[k] for k in list(d)[4:]] == ['camera', None, None, 1.25, 2.0, 300.0, None, 1.0, 100.0, 8.0, 0.3, 4e6, True]
    h = {k: v.default for k, v in inspect.signature(MH.predict_boxes).parameters.items()}
    assert all(h[k] == d[k] for k in list(d)[4:])
    assert FR.PredictedBoxes._fields == ('boxes', 'frame_index', 'track_index', 'track_id', 'detection', 'n_joints', 'n_predicted',
                                         'n_suppressed', 'n_bad_detections', 'dense_boxes', 'dense_joints')
    for word in ('design choices, not measurements', 'expand', 'n_sigma', 'max_sigma_mm', 'near_mm', 'min_side_px', 'iou_max'):
        assert word in FR.predict_boxes_in_frames.__doc__ and word in MH.predict_boxes.__doc__
    import metro_pose3d_amd
    assert metro_pose3d_amd.predict_boxes_in_frames is FR.predict_boxes_in_frames and metro_pose3d_amd.frame_sizes is FR.frame_sizes
    assert {'predict_boxes_in_frames', 'frame_sizes'} <= set(metro_pose3d_amd.__all__)

    good = FR.new_track_table(4, 17, 'cpu')
    cam = PB.pinhole()
    call = lambda tracks=good, cameras=cam, sizes=((1280, 720),), ts=(0.1,), **kw: FR.predict_boxes_in_frames(tracks, cameras, sizes, ts, **kw)
    with pytest.raises(ValueError, match="'camera' or 'world'"):
        call(coords='crop')
    for bad in ((good.state, good.ids), (good.state.float(), good.ids, good.next_id), good.state, (good.state, good.ids.long(), good.next_id)):
        with pytest.raises(ValueError, match='tracks must be'):
            call(tracks=bad)
    with pytest.raises(ValueError, match='cameras'):
        call(cameras=None)
    with pytest.raises(ValueError, match='cameras'):
        call(cameras=[cam], sizes=((1280, 720),) * 2, ts=(0.1, 0.2))
    for bad in ((), ((1280, 720, 3),), ((1280, 720),) * 65):
        with pytest.raises(ValueError, match='frame_sizes'):
            call(sizes=bad, ts=(0.1,) * len(bad))
    for bad in (((0, 720),), ((1280, -1),), ((1280.0, 720.0),)):
        with pytest.raises(ValueError, match='frame_sizes'):
            call(sizes=bad)
    for bad in ((0.1, 0.2), (), (float('nan'),), (float('inf'),)):
        with pytest.raises(ValueError, match='times must hold'):
            call(ts=bad)
    nan, inf = float('nan'), float('inf')
    for key, bads in (('expand', (0.99, nan, inf, '1', True, None)), ('n_sigma', (-0.1, nan, inf, '1', True)),
                      ('max_sigma_mm', (-1.0, nan, inf, None)), ('near_mm', (0, -1.0, nan, inf)), ('min_side_px', (-1.0, nan, inf)),
                      ('iou_max', (0, 1.01, -0.3, nan, inf, '0.3')), ('accel_psd', (0, -1.0, nan, inf)),
                      ('max_age_s', (-0.1, nan, inf, '1', None)), ('min_joints', (0, -1, 2.5, True, '3', 18))):
        for bad in bads:
            with pytest.raises(ValueError, match=key):
                call(**{key: bad})
    with pytest.raises(ValueError, match=r'detections must be'):
        call(detections=np.zeros((3, 5)))
    with pytest.raises(ValueError, match=r'detections must be'):
        call(detections=torch.zeros(4))
    with pytest.raises(ValueError, match='at most 4096'):
        call(detections=np.zeros((4097, 4)))
    with pytest.raises(ValueError, match='detection_frame_index'):
        call(detections=np.zeros((3, 4)), detection_frame_index=[0, 0])
    with pytest.raises(ValueError, match='detection_frame_index'):
        call(detections=np.zeros((3, 4)), detection_frame_index=[0.0, 0.0, 0.0])
    with pytest.raises(ValueError, match='CUDA device'):
        call()                                              # every argument fine: still no CPU path, and no launch
    # heads.predict_boxes: its own checks of the table and the camera table
    rec = FR.pack_frame_cameras(cam)
    run = lambda state=good.state, ids=good.ids, cameras=rec, **kw: MH.predict_boxes(state, ids, cameras, [[1280, 720]], [0.1], **kw)
    with pytest.raises(ValueError, match='state must be'):
        run(state=torch.zeros((129, 17, 28), dtype=torch.float64), ids=torch.zeros(129, dtype=torch.int32))
    with pytest.raises(ValueError, match='state must be'):
        run(state=torch.zeros((4, 65, 28), dtype=torch.float64))
    with pytest.raises(ValueError, match='ids must be'):
        run(ids=good.ids[:3])
    with pytest.raises(ValueError, match='cameras must be'):
        run(cameras=np.zeros(1))
    with pytest.raises(ValueError, match='cameras: 2 entries'):
        run(cameras=np.concatenate([rec, rec]))
    with pytest.raises(ValueError, match="'camera' or 'world'"):
        run(coords='crop')
    assert MH.prediction_params(1.25, 2.0, 300.0, None, 1.0, 100.0, 8.0, 0.3, 4e6) == ((4e6, 1.0, 1.25, 2.0, 300.0, 100.0, 8.0), 0.3)


# ---- the C entry ------------------------------------------------------------------------------------------------------------------

def test_new_symbol_in_header_bindings_and_library(lib):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'metro_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(metro_[a-z0-9_]+)\s*\(', text))
    name = 'metro_predict_boxes'
    assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
    params = re.search(r'\b' + name + r'\s*\(([^)]*)\)', text).group(1)
    assert len(_lib.SIGNATURES[name][1]) == params.count(',') + 1 == 33
    assert re.search(r'#define\s+METRO_PREDICT_MAX_DETECTIONS\s+4096\b', text)
    assert _lib.METRO_PREDICT_MAX_DETECTIONS == MH.PREDICT_MAX_DETECTIONS == 4096
    assert lib.metro_abi_version() == 8                    # the ABI is additive
    from metro_pose3d_amd import build
    assert 'predict_boxes.hip' in build.SOURCES and 'smooth_step.h' in build.HEADERS


def test_c_entry_rejects_bad_arguments(lib):
    """Every return below comes before any launch: no device is needed."""
    p = C.c_void_p(256)
    sizes, times = (C.c_int32 * 4)(1280, 720, 640, 480), (C.c_double * 2)(0.1, 0.2)
    fn = lib.metro_predict_boxes
    good = [p, p, 4, 17, p, 2, sizes, times, 2, _lib.METRO_COORDS_WORLD, 4e6, 1.0, 1.25, 2.0, 300.0, 100.0, 8.0, 9, 1, p, p, 8, 0.3,
            p, p, p, p, p, p, p, p, p, None]

    def call(**changes):
        a = list(good)
        for k, v in changes.items():
            a[int(k[1:])] = v
        return fn(*a)
    for nj in (0, 65, -1):
        assert call(a3=nj) == -1 and b'n_joints_out' in lib.metro_last_error()
    for bad in (_lib.METRO_COORDS_CROP, 3, -1):
        assert call(a9=bad) == -1 and b'coords' in lib.metro_last_error()
    for bad in (0, -1, 129):
        assert call(a2=bad) == -1 and b'track slots' in lib.metro_last_error()
    for bad in (0, -1, 65):
        assert call(a8=bad) == -1 and b'frames' in lib.metro_last_error()
    for bad in (-1, 4097):
        assert call(a21=bad) == -1 and b'detections' in lib.metro_last_error()
    nan, inf = float('nan'), float('inf')
    for k, word, bads in ((10, b'q must', (0.0, -1.0)), (11, b'max_age_s', (-1.0,)), (12, b'expand', (0.99, 0.0)), (13, b'n_sigma', (-0.5,)),
                          (14, b'max_sigma_mm', (-1.0,)), (15, b'near_mm', (0.0, -1.0)), (16, b'min_side_px', (-1.0,)),
                          (22, b'iou_max', (0.0, 1.5, -0.1))):
        for bad in bads + (nan, inf, -inf):
            assert call(**{f'a{k}': bad}) == -1 and word in lib.metro_last_error(), (k, bad)
    for bad in (0, 18, -1):
        assert call(a17=bad) == -1 and b'min_joints' in lib.metro_last_error()
    for bad in (0, 3):
        assert call(a5=bad) == -1 and b'cameras for' in lib.metro_last_error()
    for k in (0, 1, 4, 6, 7, 23, 24, 25, 26, 27, 28, 29, 30, 31):
        assert call(**{f'a{k}': None}) == -1 and b'NULL state' in lib.metro_last_error(), k
    for k in (19, 20):
        assert call(**{f'a{k}': None}) == -1 and b'detections with a NULL' in lib.metro_last_error()
    for bad in ((C.c_int32 * 4)(1280, 0, 640, 480), (C.c_int32 * 4)(1280, 720, -5, 480)):
        assert call(a6=bad) == -1 and b'pixels' in lib.metro_last_error()
    for bad in (nan, inf):
        assert call(a7=(C.c_double * 2)(0.1, bad)) == -1 and b'not finite' in lib.metro_last_error()
    # nothing to do: no rows can come out, no launch, whatever the pointers
    nothing = dict(a0=None, a1=None, a4=None, a6=None, a7=None, a19=None, a20=None, a21=0, **{f'a{k}': None for k in range(23, 32)})
    assert call(a2=0, **nothing) == 0 and call(a8=0, a5=0, **nothing) == 0
    assert call(a2=0) == -1 and call(a8=0) == -1, 'detections without frames or slots to hold them against'
    assert call(a2=0, a3=0, **nothing) == -1 and call(a8=0, a12=0.5, **nothing) == -1, 'a bad argument is one even then'
