"""Cross-view association without a GPU: the fp64 restatement the GPU tests compare against (tests/match_views_ref.py) on known
answers, the kernels' own per-pair and per-step code compiled for the host against that restatement, the CSR grouping against
frames.person_groups, the argument checks of the Python surface that run before any device is touched, and the new C symbols in
header, bindings and library with their invalid-argument returns."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from metro_pose3d_amd import ModelSpec, _lib, frames as FR, heads as MH
from tests import match_views_ref as MR
from tests import triangulation_ref as TR
from tests.helpers import compile_for_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC = ModelSpec(50, 32, 'h36m')
SK = SPEC.skeleton
CASES, CLUSTER_CASES = MR.CASES, MR.cluster_cases()


# ---- known answers for the restatement -------------------------------------------------------------------------------------

def test_closest_approach_of_two_rays_with_a_known_common_perpendicular():
    """Ray a runs along x through the origin, ray b along y through (3, -4, 7): they are closest at (3, 0, 0) and (3, 0, 7),
    7 apart, at ta = 3 and tb = 4.  The same after a rigid motion; b reversed meets behind its origin (tb = -4)."""
    da, oa, db, ob = np.array([1.0, 0, 0]), np.zeros(3), np.array([0, 1.0, 0]), np.array([3.0, -4.0, 7.0])
    assert np.allclose(MR.closest_approach(da, oa, db, ob), (3.0, 4.0, 7.0), rtol=0, atol=1e-12)
    assert np.allclose(MR.closest_approach(da, oa, -db, ob), (3.0, -4.0, 7.0), rtol=0, atol=1e-12)
    rot = np.linalg.qr(np.random.default_rng(0).normal(size=(3, 3)))[0]
    shift = np.array([1000.0, -2000.0, 500.0])
    got = MR.closest_approach(rot @ da, rot @ oa + shift, rot @ db, rot @ ob + shift)
    assert np.allclose(got, (3.0, 4.0, 7.0), rtol=0, atol=1e-9)


# the rigs of the known-answer test: camera angles, persons, the spacing of their centres in mm (>= 0.5 m)
EXACT_RIGS = [([0, 90], 3, 700.0), ([0, 120, 240], 5, 700.0), ([0, 70, 140, 230], 4, 700.0)]


@pytest.mark.parametrize('angles,persons,spacing', EXACT_RIGS, ids=['2-cameras', '3-cameras', '4-cameras'])
@pytest.mark.parametrize('weights', ['uniform', 'covariance'])
def test_restatement_separates_the_persons_of_an_exact_rig(angles, persons, spacing, weights):
    """Exact projections of joint clouds (sigma 300 mm) whose centres stand `spacing` apart: the rays of one person's boxes
    pass within 1e-2 mm (the fp32 rounding of the records, the triangulation tests' bound), the boxes of different persons
    cost more than the default max_cost_mm, and the clustering of that matrix recovers the persons.
    The rig was fixed on the restatement alone, before any kernel ran: the ray distance does not grow with the persons' distance
    (it sees only the part of the joints' offset that is normal to the two cameras' epipolar plane), so with random clouds the
    lowest different-person cost varies with the draw -- 190 to 310 mm over seeds 1 to 7 of the 4-camera rig; seed 2 is one
    where every pair clears 200 mm in both weight modes."""
    s = MR.rig_scene(angles, persons, SPEC, seed=2, spacing=spacing)
    c = MR.case(s, SPEC, weights)
    cost, n_pairs = MR.expected(c, SPEC)
    other_frame = c['fi'][:, None] != c['fi'][None, :]
    same = (c['pi'][:, None] == c['pi'][None, :]) & other_frame
    different = (c['pi'][:, None] != c['pi'][None, :]) & other_frame
    apart = np.linalg.norm(s['centres'][c['pi']][:, None] - s['centres'][c['pi']][None, :], axis=-1)
    assert (apart[different] >= 500.0).all()
    print(f'{len(angles)} cameras x {persons} persons, {weights}: same person <= {cost[same].max():.2e} mm, different persons >= '
          f'{cost[different].min():.1f} mm')
    assert cost.dtype == np.float32 and n_pairs.dtype == np.int32 and (n_pairs[other_frame] == SK.n_out).all()
    assert cost[same].max() <= MR.KNOWN_ANSWER_MM
    assert cost[different].min() > MR.MAX_COST_MM
    assert np.isposinf(cost[~other_frame]).all() and (n_pairs[~other_frame] == 0).all()
    labels, n_persons, rows, starts = MR.cluster(cost, MR.MAX_COST_MM)
    assert n_persons == persons and np.array_equal(labels, c['pi'])      # camera-major boxes: the lowest boxes are camera 0's
    want_rows, want_starts = FR.person_groups(c['pi'], c['fi'])
    assert np.array_equal(rows[:len(want_rows)], want_rows) and np.array_equal(starts[:persons + 1], want_starts)


# ---- the kernels' own code on the host ---------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def host_kernel(tmp_path_factory):
    """match_views.hip's per-pair function and clustering steps are __host__ __device__: the source compiled for the host, one
    call per entry of the n x n index space where the launch has one thread, and the clustering steps run by one thread."""
    tmp = tmp_path_factory.mktemp('host_match_views')
    dll = compile_for_host(tmp, 'host_match_views', ['match_views.hip'], '''
#include <vector>
extern "C" void host_view_affinity(const float* coords01, const float* cov01, const MetroPlacement* rec, const MetroSpec* spec,
                                   const int* mirror, const int* frame_index, int n, int n_views, int weights, double min_sin2,
                                   double clip_mm, int min_pairs, float* cost, int* n_pairs) {
    const metro::MatchArgs a = metro::make_match_args(coords01, cov01, rec, *spec, mirror, frame_index, n, n_views, weights,
                                                      min_sin2, clip_mm, min_pairs, cost, n_pairs);
    for (int idx = 0; idx < n * n; ++idx) metro::view_affinity_entry(a, idx);
}
extern "C" void host_cluster_views(const float* cost, int n, int n_views, float max_cost, int* person_index, int* n_persons,
                                   int* rows, int* starts) {
    using namespace metro;
    ClusterArgs a;
    a.cost = cost; a.person_index = person_index; a.n_persons = n_persons; a.rows = rows; a.starts = starts;
    a.n = n; a.n_views = n_views; a.max_cost = max_cost;
    std::vector<float> c(METRO_MATCH_MAX_BOXES * MATCH_LD);
    std::vector<int> label(n), size(n), pid(n);
    cluster_load(a, c.data(), label.data(), 0, 1);
    for (int round = 1; round < n; ++round) {
        const MatchCand best = cluster_scan(c.data(), n, 0, 1);
        if (!(best.v < max_cost)) break;
        cluster_merge(c.data(), label.data(), n, best.idx / n, best.idx % n, 0, 1);
    }
    cluster_sizes(label.data(), size.data(), n, 0, 1);
    cluster_persons(a, label.data(), size.data(), pid.data(), 0, 1);
    cluster_groups(a, label.data(), size.data(), pid.data(), 0, 1);
}
''')
    aff, clu = dll.host_view_affinity, dll.host_cluster_views
    aff.restype = clu.restype = None
    aff.argtypes = [C.c_void_p] * 3 + [C.POINTER(_lib.MetroSpec), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double,
                                       C.c_double, C.c_int, C.c_void_p, C.c_void_p]
    clu.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float] + [C.c_void_p] * 4
    ptr = lambda a: C.c_void_p(a.ctypes.data)

    def affinity(c):
        n = len(c['fi'])
        rec = np.ascontiguousarray(FR.pack_placements(c['places']))
        mirror = np.asarray(SK.out_mirror, np.int32)
        fi = np.ascontiguousarray(c['fi'], np.int32)
        cost = np.full((n, n), -7.0, np.float32)
        n_pairs = np.full((n, n), -7, np.int32)
        cs = SPEC.to_c(1)
        aff(ptr(c['coords01']), ptr(c['cov01']), ptr(rec), C.byref(cs), ptr(mirror), ptr(fi), n, c['n_views'],
            MH.TRI_WEIGHTS[c['weights']], float(np.sin(np.radians(c['min_angle_deg'])) ** 2), c['clip_mm'], MR.min_pairs_of(c, SPEC),
            ptr(cost), ptr(n_pairs))
        return cost, n_pairs

    def cluster(cost, max_cost, n_views):
        cost = np.ascontiguousarray(cost, np.float32)
        n = len(cost)
        person_index, n_persons = np.full(n, -7, np.int32), np.full(1, -7, np.int32)
        rows, starts = np.full(n * n_views, -7, np.int32), np.full(n + 1, -7, np.int32)
        clu(ptr(cost), n, n_views, max_cost, ptr(person_index), ptr(n_persons), ptr(rows), ptr(starts))
        return person_index, int(n_persons[0]), rows, starts
    return affinity, cluster


@pytest.mark.parametrize('name', list(CASES))
@pytest.mark.parametrize('weights', ['uniform', 'covariance'])
def test_pair_code_on_the_host_matches_the_restatement(host_kernel, name, weights):
    """Finite costs within 1e-3 mm of the restatement (both sides fp64 on identical fp32 inputs: the bound the triangulation
    kernel's host build is held to), equal n_pairs, +inf at the same entries, every entry written over its sentinel."""
    c = CASES[name](SPEC, weights)
    want = MR.expected(c, SPEC)
    got = host_kernel[0](c)
    worst = MR.compare(got, want, MR.PARITY_MM)
    print(f'{name}, {weights}: {len(c["fi"])} boxes, worst cost deviation {worst:.2e} mm vs the fp64 restatement')
    MR.check_case(name, c, got, SPEC)


def test_min_joints_admits_the_pairs_the_default_refuses(host_kernel):
    c = CASES['too-few'](SPEC, 'uniform')
    c['min_joints'] = 8
    got = host_kernel[0](c)
    MR.compare(got, MR.expected(c, SPEC), MR.PARITY_MM)
    others = np.flatnonzero(c['fi'] != c['fi'][0])
    assert (got[1][0, others] == 8).all() and np.isfinite(got[0][0, others]).all()


@pytest.mark.parametrize('name', list(CLUSTER_CASES))
def test_cluster_steps_on_the_host_match_the_restatement(host_kernel, name):
    """Labels, n_persons, rows and starts equal the restatement's, the labels are what the case is there to show, and the CSR is
    frames.person_groups' for those labels under frame indices that make every +inf entry a same-frame pair."""
    cost, max_cost, n_views, shown = CLUSTER_CASES[name]
    want = MR.cluster(cost, max_cost, n_views)
    got = host_kernel[1](cost, max_cost, n_views)
    MR.compare_clusters(got, want)
    labels, n_persons, rows, starts = got
    assert list(labels) == list(shown) and n_persons == max(shown) + 1
    fi = MR._frames_for(cost)
    sym = np.maximum(np.where(np.isnan(cost), np.inf, cost), np.where(np.isnan(cost.T), np.inf, cost.T))
    off = ~np.eye(len(cost), dtype=bool)
    assert np.array_equal(np.isinf(sym) & off, (fi[:, None] == fi[None, :]) & off)
    g_rows, g_starts = FR.person_groups(labels, fi, n_views)
    assert np.array_equal(rows[:len(g_rows)], g_rows) and (rows[len(g_rows):] == -1).all()
    assert np.array_equal(starts[:n_persons + 1], g_starts) and (starts[n_persons:] == len(g_rows)).all()
    if name == 'chain':
        assert MR.single_linkage(cost, max_cost) == [0, 0, 0]          # what single linkage would have joined


# ---- the surface ---------------------------------------------------------------------------------------------------------

def test_python_surface():
    sig = inspect.signature(FR.match_poses_in_frames)
    assert list(sig.parameters) == ['frames', 'boxes', 'model_path', 'cameras', 'frame_index', 'max_cost_mm', 'clip_mm', 'min_joints',
                                    'weights', 'min_angle_deg', 'views', 'precision', 'check_finite', 'geometry', 'pixel_format',
                                    'color_matrix', 'crop_dtype']
    defaults = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(max_cost_mm=200.0, clip_mm=500.0, min_joints=None, weights='covariance', min_angle_deg=2.0, views=None,
                            precision=None, check_finite=None, geometry='auto', pixel_format='rgb', color_matrix='bt601',
                            crop_dtype='float32')
    assert FR.MatchedPoses._fields == ('person_index', 'cost', 'n_pairs', 'world')
    sig = inspect.signature(MH.view_affinity)
    assert list(sig.parameters) == ['coords01', 'cov01', 'places', 'frame_index', 'spec', 'n_views', 'weights', 'min_angle_deg',
                                    'clip_mm', 'min_joints']
    assert [sig.parameters[k].default for k in ('n_views', 'weights', 'min_angle_deg', 'clip_mm', 'min_joints')] == \
        [1, 'covariance', 2.0, 500.0, None]
    sig = inspect.signature(MH.cluster_views)
    assert list(sig.parameters) == ['cost', 'max_cost_mm', 'n_views'] and sig.parameters['n_views'].default == 1
    import metro_pose3d_amd
    assert metro_pose3d_amd.match_poses_in_frames is FR.match_poses_in_frames
    assert 'match_poses_in_frames' in metro_pose3d_amd.__all__
    # the shared chain left triangulate_poses_in_frames' surface alone
    assert list(inspect.signature(FR.triangulate_poses_in_frames).parameters)[:6] == ['frames', 'boxes', 'model_path', 'cameras',
                                                                                      'person_index', 'frame_index']
    assert FR.WorldPoses._fields == ('poses', 'n_rays', 'residual', 'keypoints2d', 'joint_edges', 'joint_names')


def test_match_poses_in_frames_checks_arguments_without_a_gpu():
    cams = TR.ring_cameras([0, 90])
    frames = [np.zeros((8, 8, 3), np.uint8)] * 2
    boxes = [[0, 0, 4, 4], [1, 1, 4, 4]]
    call = lambda cameras=cams, fi=(0, 1), boxes=boxes, **kw: FR.match_poses_in_frames(frames, boxes, 'no-such-model.npz', cameras,
                                                                                       fi, **kw)
    with pytest.raises(ValueError, match='calibrated cameras'):
        call(cameras=None)
    with pytest.raises(ValueError, match='one Camera for several frames'):
        call(cameras=cams[0])
    with pytest.raises(ValueError, match='one value per box'):
        call(fi=(0,))
    with pytest.raises(ValueError, match='one value per box'):
        call(fi=(0, 1, 1))
    for fi in ((0, 2), (-1, 0)):
        with pytest.raises(ValueError, match='frame_index must lie in'):
            call(fi=fi)
    with pytest.raises(ValueError, match='at most 128'):
        call(boxes=np.tile([[0.0, 0, 4, 4]], (129, 1)), fi=np.arange(129) % 2)
    for name in ('max_cost_mm', 'clip_mm'):
        for bad in (0, -1.0, float('nan'), float('inf'), '200', True, None):
            with pytest.raises(ValueError, match=name):
                call(**{name: bad})
    for bad in (0, -1.0, 90.5, float('nan'), '2', True):
        with pytest.raises(ValueError, match='min_angle_deg'):
            call(min_angle_deg=bad)
    for bad in (0, -3, 2.5, '9', True):
        with pytest.raises(ValueError, match='min_joints'):
            call(min_joints=bad)
    for bad in ('huber', None, 1):
        with pytest.raises(ValueError, match='weights must be'):
            call(weights=bad)


def test_heads_functions_check_arguments_before_the_library_or_a_device():
    m, nj = 4, SK.n_head
    c01, cov = torch.zeros((m, nj, 3)), torch.zeros((m, nj, 6))
    places = torch.zeros(m * C.sizeof(_lib.MetroPlacement), dtype=torch.uint8)
    fi = [0, 1, 0, 1]
    with pytest.raises(ValueError, match='weights must be'):
        MH.view_affinity(c01, cov, places, fi, SPEC, weights='robust')
    with pytest.raises(ValueError, match='min_angle_deg'):
        MH.view_affinity(c01, cov, places, fi, SPEC, min_angle_deg=0)
    with pytest.raises(ValueError, match='clip_mm'):
        MH.view_affinity(c01, cov, places, fi, SPEC, clip_mm=0)
    for bad in (0, SK.n_out + 1, 1.5):
        with pytest.raises(ValueError, match='min_joints'):
            MH.view_affinity(c01, cov, places, fi, SPEC, min_joints=bad)
    with pytest.raises(ValueError, match='coords01 must be'):
        MH.view_affinity(c01[..., :2], cov, places, fi, SPEC)
    with pytest.raises(ValueError, match='needs cov01'):
        MH.view_affinity(c01, None, places, fi, SPEC)
    with pytest.raises(ValueError, match='MetroPlacement'):
        MH.view_affinity(c01, cov, places[:-1], fi, SPEC)
    with pytest.raises(ValueError, match='one value per box'):
        MH.view_affinity(c01, cov, places, fi[:3], SPEC)
    with pytest.raises(ValueError, match='one value per box'):
        MH.view_affinity(c01, cov, places, fi, SPEC, n_views=2)
    for bad in (0, 33, 3, 1.0):
        with pytest.raises(ValueError, match='views'):
            MH.view_affinity(c01, cov, places, fi, SPEC, n_views=bad)
    big = 129
    with pytest.raises(ValueError, match='at most 128'):
        MH.view_affinity(torch.zeros((big, nj, 3)), None, torch.zeros(big * C.sizeof(_lib.MetroPlacement), dtype=torch.uint8),
                         [0] * big, SPEC, weights='uniform')
    with pytest.raises(ValueError, match='at most 128'):
        MH.cluster_views(torch.zeros((big, big)), 200.0)
    for bad in (0, -1.0, float('nan'), '200', None):
        with pytest.raises(ValueError, match='max_cost_mm'):
            MH.cluster_views(torch.zeros((2, 2)), bad)
    with pytest.raises(ValueError, match='square'):
        MH.cluster_views(torch.zeros((2, 3)), 200.0)
    with pytest.raises(ValueError, match='n_views'):
        MH.cluster_views(torch.zeros((2, 2)), 200.0, n_views=0)


def test_new_symbols_in_header_bindings_and_library(lib):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'metro_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(metro_[a-z0-9_]+)\s*\(', text))
    for name, n_args in (('metro_view_affinity', 15), ('metro_cluster_views', 9)):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
        params = re.search(r'\b' + name + r'\s*\(([^)]*)\)', text).group(1)
        assert len(_lib.SIGNATURES[name][1]) == params.count(',') + 1 == n_args
    assert re.search(r'#define\s+METRO_MATCH_MAX_BOXES\s+128\b', text)
    assert _lib.METRO_MATCH_MAX_BOXES == MH.MATCH_MAX_BOXES == MR.MAX_BOXES == 128
    assert 'match_views.hip' in __import__('metro_pose3d_amd.build', fromlist=['SOURCES']).SOURCES
    assert lib.metro_abi_version() == 8                    # the ABI is additive


def test_c_entries_reject_bad_arguments(lib):
    """Every return below comes before any launch: no device is needed."""
    cs = SPEC.to_c(_lib.METRO_PREC_F16)
    p, s2 = C.c_void_p(256), float(np.sin(np.radians(2.0)) ** 2)
    aff, clu = lib.metro_view_affinity, lib.metro_cluster_views
    good = [p, p, p, C.byref(cs), p, p, 4, 1, _lib.METRO_TRI_COVARIANCE, s2, 500.0, 9, p, p, None]

    def call(fn, base, **changes):
        a = list(base)
        for k, v in changes.items():
            a[int(k[1:])] = v
        return fn(*a)
    assert call(aff, good, a3=None) == -1 and b'spec' in lib.metro_last_error()
    for w in (-1, 2):
        assert call(aff, good, a8=w) == -1 and b'weights' in lib.metro_last_error()
    assert call(aff, good, a6=-1) == -1 and b'negative' in lib.metro_last_error()
    assert call(aff, good, a6=129) == -1 and b'at most 128' in lib.metro_last_error()
    for v in (0, 33):
        assert call(aff, good, a7=v) == -1 and b'views' in lib.metro_last_error()
    for v in (0.0, -0.1, 1.5, float('nan')):
        assert call(aff, good, a9=v) == -1 and b'min_sin2' in lib.metro_last_error()
    for v in (0.0, -1.0, float('nan')):
        assert call(aff, good, a10=v) == -1 and b'clip_mm' in lib.metro_last_error()
    assert call(aff, good, a11=0) == -1 and b'min_pairs' in lib.metro_last_error()
    assert call(aff, good, a1=None) == -1 and b'cov01' in lib.metro_last_error()
    assert call(aff, good, a1=None, a8=_lib.METRO_TRI_UNIFORM, a6=0) == 0
    for k in (0, 2, 4, 5, 12, 13):                         # coords01, records, mirror, frame_index, the two outputs
        assert call(aff, good, **{f'a{k}': None}) == -1 and b'NULL' in lib.metro_last_error()
    # no boxes: nothing to launch, whatever the pointers
    assert aff(None, None, None, C.byref(cs), None, None, 0, 1, _lib.METRO_TRI_COVARIANCE, s2, 500.0, 9, None, None, None) == 0
    good = [p, 4, 1, 200.0, p, p, p, p, None]
    assert call(clu, good, a1=-1) == -1 and b'negative' in lib.metro_last_error()
    assert call(clu, good, a1=129) == -1 and b'at most 128' in lib.metro_last_error()
    for v in (0, 33):
        assert call(clu, good, a2=v) == -1 and b'views' in lib.metro_last_error()
    for v in (0.0, -5.0, float('nan')):
        assert call(clu, good, a3=v) == -1 and b'max_cost' in lib.metro_last_error()
    for k in (0, 4, 5, 6, 7):
        assert call(clu, good, **{f'a{k}': None}) == -1 and b'NULL' in lib.metro_last_error()
    assert clu(None, 0, 1, 200.0, None, None, None, None, None) == 0
