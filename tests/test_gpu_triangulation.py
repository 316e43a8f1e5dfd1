"""metro_triangulate_joints and frames.triangulate_poses_in_frames on the MI355X: the kernel against its fp64 restatement
(tests/triangulation_ref.py) on the same fp32 inputs -- ragged and scrambled groups across a block boundary, a flipped
test-time view, skipped and dropped rays, undetermined joints -- the empty calls, and the whole call against
heads.triangulate_joints on the chain's own intermediates."""
import ctypes as C

import numpy as np
import pytest
import torch

from metro_pose3d_amd import ModelSpec, _lib, frames as FR, heads as MH
from metro_pose3d_amd._lib import check
from tests import triangulation_ref as TR

pytestmark = pytest.mark.gpu

SPEC = ModelSpec(50, 32, 'h36m')
SK = SPEC.skeleton
SENTINEL = -7.0
CASES, KNOWN_ANSWER_MM, PARITY_MM = TR.CASES, TR.KNOWN_ANSWER_MM, TR.PARITY_MM


def _device_case(c, cuda):
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    return dict(coords01=up(c['coords01']), cov01=up(c['cov01']), places=up(FR.pack_placements(c['places'])).reshape(-1),
                rows=up(c['rows']), starts=up(c['starts']))


def _launch(d, c, cuda):
    """One metro_triangulate_joints call into outputs pre-filled with a sentinel -> (points, n_rays, residual) NumPy arrays."""
    n_persons = len(c['starts']) - 1
    points = torch.full((n_persons, SK.n_out, 3), SENTINEL, dtype=torch.float32, device=cuda)
    n_rays = torch.full((n_persons, SK.n_out), int(SENTINEL), dtype=torch.int32, device=cuda)
    residual = torch.full((n_persons, SK.n_out), SENTINEL, dtype=torch.float32, device=cuda)
    mirror = torch.from_numpy(np.asarray(SK.out_mirror, np.int32)).to(cuda)
    cs = SPEC.to_c(1)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    check(_lib.load().metro_triangulate_joints(
        ptr(d['coords01']), ptr(d['cov01']), ptr(d['places']), len(c['coords01']), ptr(d['rows']), len(c['rows']), ptr(d['starts']),
        n_persons, C.byref(cs), ptr(mirror), MH.TRI_WEIGHTS[c['weights']], TR.min_det(c['min_angle_deg']), ptr(points), ptr(n_rays),
        ptr(residual), C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)), 'metro_triangulate_joints')
    return points.cpu().numpy(), n_rays.cpu().numpy(), residual.cpu().numpy()


@pytest.mark.parametrize('name', list(CASES))
@pytest.mark.parametrize('weights', ['uniform', 'covariance'])
def test_kernel_matches_the_restatement(cuda, name, weights):
    """Points and residuals within 1e-3 mm of the restatement (both sides fp64 on identical fp32 inputs), equal ray counts, equal
    NaN pattern, every output written over its sentinel; then what the case is there to show (TR.check_case): the ragged
    groups' counts, the mirror swap of the flipped view, the skipped and the dropped rays, the undetermined joints next to
    untouched ones.  The `ragged` case has 4 persons x 17 joints = 68 threads: two blocks."""
    c = CASES[name](SPEC, weights)
    want = TR.expected(c, SPEC)
    d = _device_case(c, cuda)
    got = _launch(d, c, cuda)
    worst = TR.compare(got, want, PARITY_MM)
    print(f'{name}, {weights}: worst point {worst[0]:.2e} mm, worst residual {worst[1]:.2e} mm vs the fp64 restatement')
    TR.check_case(name, c, got, KNOWN_ANSWER_MM)
    # the thin binding is this launch
    points, n_rays, residual = MH.triangulate_joints(d['coords01'], d['cov01'], d['places'], c['rows'], c['starts'], SPEC, weights,
                                                     c['min_angle_deg'])
    assert points.dtype == torch.float32 and n_rays.dtype == torch.int32 and points.device.type == 'cuda'
    for a, b in zip((points, n_rays, residual), got):
        assert np.array_equal(a.cpu().numpy(), b, equal_nan=True)


def test_covariance_weights_move_the_point_towards_the_certain_rays(cuda):
    """The weights test of tests/test_triangulation.py on the kernel: a 20 px displacement declared with sigma^2 = 400 px^2 costs
    the covariance solve less than a tenth of what it costs the uniform solve."""
    s = TR.ring_scene([0, 120, 240], 2, SPEC, seed=2)
    n, lrc = len(s['boxes']), TR.pixel_scale(SPEC)[0]
    coords01 = s['coords01'].copy()
    coords01[1, SK.permutation[0], 0] += np.float32(20.0 / lrc)
    var = np.ones((n, SK.n_head))
    var[1, SK.permutation[0]] = 400.0
    rows, starts = FR.person_groups(s['pi'], s['fi'])
    err = {}
    for weights in ('uniform', 'covariance'):
        c = TR.case(coords01, TR.cov01_for(var, SPEC, (n, SK.n_head)), s['places'], rows, starts, weights)
        got = _launch(_device_case(c, cuda), c, cuda)
        TR.compare(got, TR.expected(c, SPEC), PARITY_MM)
        e = np.linalg.norm(got[0] - s['truth'], axis=-1)
        err[weights] = e[0, 0]
        e[0, 0] = 0
        assert e.max() <= KNOWN_ANSWER_MM
    print(f"displaced joint: uniform {err['uniform']:.2f} mm, covariance {err['covariance']:.2f} mm")
    assert err['uniform'] > 10 and err['covariance'] < 0.1 * err['uniform']


def test_no_persons_and_no_boxes_launch_nothing(cuda, tmp_path):
    lib = _lib.load()
    cs = SPEC.to_c(1)
    assert lib.metro_kernel_notes(1) == 0
    try:
        st = lib.metro_triangulate_joints(None, None, None, 0, None, 0, None, 0, C.byref(cs), None, _lib.METRO_TRI_COVARIANCE,
                                          TR.min_det(2.0), None, None, None, None)
        empty = lambda *s: torch.empty(s, device=cuda)
        points, n_rays, residual = MH.triangulate_joints(empty(0, SK.n_head, 3), empty(0, SK.n_head, 6),
                                                         torch.empty(0, dtype=torch.uint8, device=cuda), [], [0], SPEC)
        from tests.test_gpu_placement import _toy_engine_model
        spec, _, path = _toy_engine_model(tmp_path)
        res = FR.triangulate_poses_in_frames([np.zeros((24, 32, 3), np.uint8)] * 2, np.zeros((0, 4)), path,
                                             TR.ring_cameras([0, 90]), [], [])
        launched = lib.metro_last_kernel_id()
    finally:
        lib.metro_kernel_notes(0)
    assert st == 0 and not launched, launched
    assert points.shape == (0, SK.n_out, 3) and n_rays.shape == (0, SK.n_out) and residual.shape == (0, SK.n_out)
    n_out = spec.skeleton.n_out
    assert res.poses.shape == (0, n_out, 3) and res.n_rays.shape == (0, n_out) and res.n_rays.dtype == torch.int32
    assert res.residual.shape == (0, n_out) and res.keypoints2d.shape == (0, n_out, 2) and res.poses.device.type == 'cuda'
    assert len(res.joint_names) == n_out and res.joint_edges.shape[1] == 2
    # persons without rows: one launch, every joint NaN with no rays
    places = torch.empty(0, dtype=torch.uint8, device=cuda)
    points, n_rays, residual = MH.triangulate_joints(empty(0, SK.n_head, 3), None, places, [], [0, 0, 0], SPEC, 'uniform')
    assert points.shape == (2, SK.n_out, 3) and torch.isnan(points).all() and torch.isnan(residual).all() and (n_rays == 0).all()


def _rig_scene():
    """3 cameras on a ring with 320 x 240 frames of noise; persons 0 and 1 boxed in every frame, person 2 in frame 0 only."""
    rng = np.random.default_rng(21)
    cams = TR.ring_cameras([0, 100, 215], focal=260.0, principal=(160.0, 120.0))
    frames = [rng.integers(0, 256, (240, 320, 3), dtype=np.uint8) for _ in cams]
    boxes = np.array([[60.0, 40, 70, 150], [170, 50, 80, 140], [50, 30, 90, 160], [180, 60, 60, 120], [90, 45, 75, 150],
                      [200, 40, 70, 160], [10, 10, 60, 100]])
    return cams, frames, boxes, np.array([0, 0, 1, 1, 2, 2, 0]), np.array([0, 1, 0, 1, 0, 1, 2])


@pytest.mark.parametrize('views', [None, 2], ids=['one-view', 'two-views'])
def test_triangulate_poses_in_frames_is_the_chain_plus_one_launch(cuda, tmp_path, views):
    """The whole call against heads.triangulate_joints on the chain's own intermediates (_warp_views, then the engine's forward
    with coords01 / cov01 / peak), bit for bit, in both weight modes; keypoints2d are locate_poses_in_frames' bits; the person
    boxed on one frame only is not solved.  f32m: its forward gives a batch the same bits in every call."""
    from metro_pose3d_amd.inference import _engine_for
    from tests.test_gpu_placement import _toy_engine_model
    spec, _, path = _toy_engine_model(tmp_path)
    sk = spec.skeleton
    cams, frames, boxes, fi, pi = _rig_scene()
    vs = FR.view_set(1 if views is None else views)
    n, nv = len(boxes), len(vs.zoom)
    m = n * nv
    with torch.cuda.device(cuda):
        eng = _engine_for(path, 'f32m', cuda, m)
        crops, places = FR._warp_views(frames, cams, boxes, fi, vs, spec.proc_side, cuda)
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=cuda)
        c01, cov, peak = f32(m, sk.n_head, 3), f32(m, sk.n_head, 6), f32(m, sk.n_head)
        eng.forward(crops, coords01=c01, cov01=cov, peak=peak)
    rows, starts = FR.person_groups(pi, fi, nv)
    assert list(starts) == [0, 3 * nv, 6 * nv, 6 * nv]
    ref = FR.locate_poses_in_frames(frames, boxes, path, cameras=cams, frame_index=fi, scale_recovery='metro', precision='f32m',
                                    views=views)
    for weights in ('covariance', 'uniform'):
        got = FR.triangulate_poses_in_frames(frames, boxes, path, cams, pi, fi, weights=weights, views=views, precision='f32m')
        want = MH.triangulate_joints(c01, cov, places.reshape(-1), rows, starts, spec, weights)
        assert got.poses.shape == (3, sk.n_out, 3) and got.n_rays.dtype == torch.int32
        for a, b in zip((got.poses, got.n_rays, got.residual), want):
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True), weights
        assert np.array_equal(got.keypoints2d.cpu().numpy(), ref.keypoints2d.cpu().numpy(), equal_nan=True)
        assert torch.isnan(got.poses[2]).all() and (got.n_rays[2] == 0).all()
        assert (got.n_rays[:2] <= 3 * nv).all()
    # device boxes: the same chain from metro_look_at_boxes' records (within an fp32 ulp of the host's, not their bits)
    geo = FR.triangulate_poses_in_frames(frames, torch.from_numpy(boxes).to(cuda), path, cams, pi, fi, views=views, precision='f32m')
    assert geo.poses.shape == (3, sk.n_out, 3) and (geo.n_rays[2] == 0).all() and torch.isnan(geo.poses[2]).all()
