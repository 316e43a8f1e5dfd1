"""metro_view_affinity, metro_cluster_views and frames.match_poses_in_frames on the MI355X: the two launches against their fp64
restatement (tests/match_views_ref.py) on the same fp32 inputs, into poisoned output buffers, at the sizes where the index space
crosses a wave and a block and fills the LDS matrix; and the whole call against the stand-alone heads functions and
triangulate_poses_in_frames on the person_index it found.  Every GPU step runs once."""
import ctypes as C

import numpy as np
import pytest
import torch

from metro_pose3d_amd import ModelSpec, _lib, frames as FR, heads as MH
from metro_pose3d_amd._lib import check
from tests import match_views_ref as MR
from tests import triangulation_ref as TR

pytestmark = pytest.mark.gpu

H36M = ModelSpec(50, 32, 'h36m')
MERGED = ModelSpec(50, 32, 'merged')                  # 19 output joints of a larger head
SENTINEL = -7


def _n65(spec, weights):
    """5 cameras x 13 persons: 65 boxes, 4225 entries = 66 waves and a 2-thread tail."""
    return MR.case(MR.rig_scene([0, 70, 140, 215, 290], 13, spec, seed=31), spec, weights, noise_px=2.0, seed=31)


def _n128(spec, weights):
    """2 cameras x 64 persons, the LDS-filling size.  The restatement solves one least-squares system per ray pair, so the
    frame indices are redrawn to keep the boxes of different frames few: 12 boxes, among them 63, 64, 65 and 127, the last, are
    on frames of their own kind (1 or 2) and the other 116 on frame 0."""
    c = MR.case(MR.rig_scene([0, 90], 64, spec, seed=32), spec, weights, noise_px=2.0, seed=32)
    fi = np.zeros(128, np.int32)
    fi[[3, 40, 63, 64, 65, 90, 126]] = 1
    fi[[0, 17, 66, 101, 127]] = 2
    c['fi'] = fi
    return c


def _views2(spec, weights):
    return MR.case(MR.rig_scene([0, 100, 200], 2, spec, seed=33, views=2), spec, weights, noise_px=1.0, seed=33)


BIG_CASES = {'n65-h36m': (_n65, H36M), 'n128-merged': (_n128, MERGED), 'views2-merged': (_views2, MERGED),
             'n2-merged': (MR.CASES['rig-2x1'], MERGED)}
AFFINITY_CASES = [(name, fn, H36M) for name, fn in MR.CASES.items()] + [(name, fn, spec) for name, (fn, spec) in BIG_CASES.items()]


def _ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _stream(cuda):
    return C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)


def _device_case(c, cuda):
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    return dict(coords01=up(c['coords01']), cov01=up(c['cov01']), places=up(FR.pack_placements(c['places'])).reshape(-1),
                fi=up(np.asarray(c['fi'], np.int32)))


def _launch_affinity(d, c, spec, cuda):
    """One metro_view_affinity call into outputs pre-filled with a sentinel -> (cost, n_pairs) NumPy arrays."""
    n = len(c['fi'])
    cost = torch.full((n, n), float(SENTINEL), dtype=torch.float32, device=cuda)
    n_pairs = torch.full((n, n), SENTINEL, dtype=torch.int32, device=cuda)
    mirror = torch.from_numpy(np.asarray(spec.skeleton.out_mirror, np.int32)).to(cuda)
    cs = spec.to_c(1)
    check(_lib.load().metro_view_affinity(
        _ptr(d['coords01']), _ptr(d['cov01']), _ptr(d['places']), C.byref(cs), _ptr(mirror), _ptr(d['fi']), n, c['n_views'],
        MH.TRI_WEIGHTS[c['weights']], float(np.sin(np.radians(c['min_angle_deg'])) ** 2), c['clip_mm'], MR.min_pairs_of(c, spec),
        _ptr(cost), _ptr(n_pairs), _stream(cuda)), 'metro_view_affinity')
    return cost.cpu().numpy(), n_pairs.cpu().numpy()


@pytest.mark.parametrize('name,build,spec', AFFINITY_CASES, ids=[a[0] for a in AFFINITY_CASES])
@pytest.mark.parametrize('weights', ['uniform', 'covariance'])
def test_view_affinity_matches_the_restatement(cuda, name, build, spec, weights):
    """Finite costs within 1e-3 mm of the restatement (both sides fp64 on identical fp32 inputs), equal n_pairs, +inf at the same
    entries, every entry written over its sentinel, the matrix symmetric; the host cases' own checks; heads.view_affinity is
    this launch."""
    c = build(spec, weights)
    want = MR.expected(c, spec)
    d = _device_case(c, cuda)
    got = _launch_affinity(d, c, spec, cuda)
    worst = MR.compare(got, want, MR.PARITY_MM)
    print(f'{name}, {weights}: {len(c["fi"])} boxes x {c["n_views"]} views, J = {spec.skeleton.n_out}: worst cost deviation '
          f'{worst:.2e} mm vs the fp64 restatement')
    if name in MR.CASES:
        MR.check_case(name, c, got, spec)
    cost, n_pairs = MH.view_affinity(d['coords01'], d['cov01'], d['places'], d['fi'], spec, c['n_views'], weights,
                                     c['min_angle_deg'], c['clip_mm'], c['min_joints'])
    assert cost.dtype == torch.float32 and n_pairs.dtype == torch.int32 and cost.device.type == 'cuda'
    assert np.array_equal(cost.cpu().numpy(), got[0]) and np.array_equal(n_pairs.cpu().numpy(), got[1])


def _launch_cluster(cost, max_cost, n_views, cuda):
    """One metro_cluster_views call into outputs pre-filled with a sentinel -> the four outputs as NumPy arrays."""
    n = len(cost)
    d_cost = torch.from_numpy(np.ascontiguousarray(cost, np.float32)).to(cuda)
    i32 = lambda k: torch.full((k,), SENTINEL, dtype=torch.int32, device=cuda)
    person_index, n_persons, rows, starts = i32(n), i32(1), i32(n * n_views), i32(n + 1)
    check(_lib.load().metro_cluster_views(_ptr(d_cost), n, n_views, max_cost, _ptr(person_index), _ptr(n_persons), _ptr(rows),
                                          _ptr(starts), _stream(cuda)), 'metro_cluster_views')
    got = tuple(t.cpu().numpy() for t in (person_index, n_persons, rows, starts))
    via_heads = MH.cluster_views(d_cost, max_cost, n_views)
    assert all(t.dtype == torch.int32 and t.device.type == 'cuda' for t in via_heads)
    MR.compare_clusters([t.cpu().numpy() for t in via_heads], got)
    return got


@pytest.mark.parametrize('name', list(MR.cluster_cases()))
def test_cluster_views_on_the_hand_made_matrices(cuda, name):
    cost, max_cost, n_views, shown = MR.cluster_cases()[name]
    got = _launch_cluster(cost, max_cost, n_views, cuda)
    MR.compare_clusters(got, MR.cluster(cost, max_cost, n_views))
    assert list(got[0]) == list(shown)


@pytest.mark.parametrize('n', [2, 63, 64, 65, 128])
def test_cluster_views_on_random_matrices(cuda, n):
    """Distinct finite values (no tie that fp32 ordering could flip; the tie rule is the hand-made cases') with 15 % of the pairs
    +inf, thresholds that stop the merging early, half way and never: all four outputs equal the restatement's."""
    cost = MR.random_cost(n, seed=n)
    for max_cost, n_views in ((60.0, 1), (200.0, 2), (1e9, 1)):
        want = MR.cluster(cost, max_cost, n_views)
        got = _launch_cluster(cost, max_cost, n_views, cuda)
        MR.compare_clusters(got, want)
        print(f'n = {n}, max_cost {max_cost:g}: {want[1]} persons, {int(want[3][-1])} grouped rows')


# ---- the whole call ----------------------------------------------------------------------------------------------------------

def _rig():
    """3 cameras on a ring with 320 x 240 frames of noise and 7 boxes in detector order (3 on frame 0, 3 on frame 1, 1 on frame 2)."""
    rng = np.random.default_rng(21)
    cams = TR.ring_cameras([0, 100, 215], focal=260.0, principal=(160.0, 120.0))
    frames = [rng.integers(0, 256, (240, 320, 3), dtype=np.uint8) for _ in cams]
    boxes = np.array([[60.0, 40, 70, 150], [50, 30, 90, 160], [90, 45, 75, 150], [170, 50, 80, 140], [180, 60, 60, 120],
                      [200, 40, 70, 160], [10, 10, 60, 100]])
    return cams, frames, boxes, np.array([0, 0, 0, 1, 1, 1, 2])


def _equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)


@pytest.mark.parametrize('precision', ['f64', 'f16'])
@pytest.mark.parametrize('views,device_boxes', [(None, False), (2, False), (None, True)], ids=['one-view', 'two-views', 'device-boxes'])
def test_match_poses_in_frames_is_the_chain_plus_two_launches(cuda, tmp_path, precision, views, device_boxes):
    """A synthetic model's poses mean nothing, so this checks plumbing and equivalence: person_index, cost and n_pairs are
    heads.cluster_views(heads.view_affinity(...)) on a forward of the same crops, and `world` is triangulate_poses_in_frames
    called with that person_index on the same inputs, bit for bit with NaNs at the same places -- in both weight modes, and
    with a max_cost_mm above clip_mm, under which every pair of boxes that has a cost may merge (so that some person has
    several boxes whatever the weights give), as well as the default."""
    from metro_pose3d_amd.inference import _engine_for
    from tests.test_gpu_placement import _toy_engine_model
    spec, _, path = _toy_engine_model(tmp_path)
    sk = spec.skeleton
    cams, frames, boxes, fi = _rig()
    vs = FR.view_set(1 if views is None else views)
    n, nv = len(boxes), len(vs.zoom)
    m = n * nv
    given = torch.from_numpy(boxes).to(cuda) if device_boxes else boxes
    kw = dict(views=views, precision=precision, geometry='device' if device_boxes else 'auto')
    with torch.cuda.device(cuda):
        eng = _engine_for(path, precision, cuda, m)
        call = FR._checked_call(frames, given, fi, 'world', views, kw['geometry'], precision, None, 'rgb', 'bt601')
        crops, places = FR._warp_views(call.frames, cams, call.boxes, call.fi, call.vs, spec.proc_side, cuda)
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=cuda)
        c01, cov, peak = f32(m, sk.n_head, 3), f32(m, sk.n_head, 6), f32(m, sk.n_head)
        eng.forward(crops, coords01=c01, cov01=cov, peak=peak)
    merged_some = False
    for weights, max_cost in (('covariance', 200.0), ('covariance', 600.0), ('uniform', 600.0)):
        got = FR.match_poses_in_frames(frames, given, path, cams, fi, max_cost_mm=max_cost, weights=weights, **kw)
        cost, n_pairs = MH.view_affinity(c01, cov, places.reshape(-1), fi, spec, nv, weights)
        labels, n_persons, rows, starts = MH.cluster_views(cost, max_cost, nv)
        assert got.person_index.dtype == torch.int32 and got.person_index.device.type == 'cuda'
        assert _equal(got.person_index, labels) and _equal(got.cost, cost) and _equal(got.n_pairs, n_pairs), (weights, max_cost)
        persons = int(n_persons.item())
        assert persons == int(labels.max().item()) + 1 and got.world.poses.shape == (persons, sk.n_out, 3)
        assert got.world.n_rays.shape == (persons, sk.n_out) and got.world.residual.shape == (persons, sk.n_out)
        want = FR.triangulate_poses_in_frames(frames, given, path, cams, labels.cpu().numpy(), fi, weights=weights, **kw)
        for field in ('poses', 'n_rays', 'residual', 'keypoints2d'):
            assert _equal(getattr(got.world, field), getattr(want, field)), (field, weights, max_cost)
        sizes = np.bincount(labels.cpu().numpy())
        assert (got.world.n_rays[torch.from_numpy(sizes == 1).to(cuda)] == 0).all()        # one box: no depth, not solved
        merged_some |= bool((sizes > 1).any() and torch.isfinite(got.world.poses).any())
        print(f'{precision}, views {views}, device boxes {device_boxes}, {weights}, max_cost {max_cost:g}: {persons} persons of '
              f'{n} boxes, sizes {sizes.tolist()}')
    assert merged_some


def test_no_boxes_launch_nothing(cuda, tmp_path):
    from tests.test_gpu_placement import _toy_engine_model
    spec, _, path = _toy_engine_model(tmp_path)
    lib = _lib.load()
    cs = spec.to_c(1)
    empty = lambda *s, dtype=torch.float32: torch.empty(s, dtype=dtype, device=cuda)
    assert lib.metro_kernel_notes(1) == 0
    try:
        st = (lib.metro_view_affinity(None, None, None, C.byref(cs), None, None, 0, 1, _lib.METRO_TRI_COVARIANCE, 0.5, 500.0, 9, None,
                                      None, None),
              lib.metro_cluster_views(None, 0, 1, 200.0, None, None, None, None, None))
        cost, n_pairs = MH.view_affinity(empty(0, spec.skeleton.n_head, 3), empty(0, spec.skeleton.n_head, 6),
                                         empty(0, dtype=torch.uint8), [], spec)
        res = FR.match_poses_in_frames([np.zeros((24, 32, 3), np.uint8)] * 2, np.zeros((0, 4)), path, TR.ring_cameras([0, 90]), [])
        launched = lib.metro_last_kernel_id()
    finally:
        lib.metro_kernel_notes(0)
    assert st == (0, 0) and not launched, launched
    n_out = spec.skeleton.n_out
    assert cost.shape == (0, 0) and n_pairs.shape == (0, 0) and n_pairs.dtype == torch.int32
    assert res.person_index.shape == (0,) and res.person_index.dtype == torch.int32 and res.person_index.device.type == 'cuda'
    assert res.cost.shape == (0, 0) and res.n_pairs.shape == (0, 0)
    assert res.world.poses.shape == (0, n_out, 3) and res.world.n_rays.shape == (0, n_out) and res.world.keypoints2d.shape == (0, n_out, 2)
