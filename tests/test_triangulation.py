"""World poses from several calibrated cameras, without a GPU: the fp64 restatement the GPU tests compare against
(tests/triangulation_ref.py) on known answers, the kernel's own per-joint code compiled for the host against that restatement,
the CSR grouping, the argument checks of the Python surface that run before any device is touched, and the new C symbol in
header, bindings and library with its invalid-argument returns."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from metro_pose3d_amd import ModelSpec, _lib, frames as FR, heads as MH
from tests import triangulation_ref as TR
from tests.helpers import compile_for_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC = ModelSpec(50, 32, 'h36m')
SK = SPEC.skeleton
KNOWN_ANSWER_MM, PARITY_MM, CASES = TR.KNOWN_ANSWER_MM, TR.PARITY_MM, TR.CASES


def _run_ref(s, weights, cov01=None, coords01=None, min_angle_deg=2.0, groups=None):
    q = s['places']
    n = len(s['boxes'])
    rows, starts = groups if groups is not None else FR.person_groups(s['pi'], s['fi'])
    cov01 = TR.cov01_for(1.0, SPEC, (n, SK.n_head)) if cov01 is None else cov01
    return TR.triangulate(s['coords01'] if coords01 is None else coords01, cov01, q.inv_intrinsics, q.rot_to_world, q.cam_loc,
                          rows, starts, SK.permutation, SK.out_mirror, SPEC, weights, min_angle_deg)


@pytest.mark.parametrize('angles', [[0, 90], [0, 120, 240], [0, 90, 180, 270]], ids=['2-cameras', '3-cameras', '4-cameras'])
@pytest.mark.parametrize('weights', ['uniform', 'covariance'])
def test_restatement_recovers_known_points(angles, weights):
    """Cameras on a ring at 4.5 m (odd ones with lens distortion), joints with sigma = 300 mm, coords01 projected through each
    crop record's own virtual camera: the points come back within 1e-2 mm."""
    s = TR.ring_scene(angles, 2, SPEC, seed=1)
    points, n_rays, residual = _run_ref(s, weights)
    err = np.abs(points - s['truth']).max()
    print(f'{len(angles)} cameras, {weights}: worst {err:.2e} mm, worst residual {residual.max():.2e} mm')
    assert (n_rays == len(angles)).all() and points.dtype == np.float32 and n_rays.dtype == np.int32
    assert err <= KNOWN_ANSWER_MM and residual.max() <= KNOWN_ANSWER_MM


def test_covariance_weights_discount_the_uncertain_ray():
    """3 cameras; camera 1 sees joint 0 of person 0 displaced by 20 px and says so (sigma^2 = 400 px^2 against 1 on every other
    ray): the covariance solve lands within a tenth of the uniform solve's error; every other joint stays within the
    known-answer bound in both modes."""
    s = TR.ring_scene([0, 120, 240], 2, SPEC, seed=2)
    n, lrc = len(s['boxes']), TR.pixel_scale(SPEC)[0]
    coords01 = s['coords01'].copy()
    coords01[1, SK.permutation[0], 0] += np.float32(20.0 / lrc)
    var = np.ones((n, SK.n_head))
    var[1, SK.permutation[0]] = 400.0
    cov01 = TR.cov01_for(var, SPEC, (n, SK.n_head))
    err = {}
    for weights in ('uniform', 'covariance'):
        points, n_rays, _ = _run_ref(s, weights, cov01, coords01)
        e = np.linalg.norm(points - s['truth'], axis=-1)
        err[weights] = e[0, 0]
        e[0, 0] = 0
        assert e.max() <= KNOWN_ANSWER_MM and (n_rays == 3).all()
    print(f"displaced joint: uniform {err['uniform']:.2f} mm, covariance {err['covariance']:.2f} mm")
    assert err['uniform'] > 10 and err['covariance'] < 0.1 * err['uniform']


def test_determinacy():
    for weights in ('uniform', 'covariance'):
        c = TR.determinacy_case(SPEC, weights)
        points, n_rays, residual = TR.expected(c, SPEC)
        undetermined = np.isnan(points).all(axis=-1)
        assert np.array_equal(undetermined, np.isnan(points).any(axis=-1)) and np.array_equal(undetermined, np.isnan(residual))
        # two rays 1 degree apart: NaN with n_rays 2 at the default 2 degrees
        assert undetermined[0].all() and (n_rays[0] == 2).all()
        # one joint with one ray: NaN, the person's other joints untouched
        assert undetermined[1].sum() == 1 and undetermined[1, 5] and n_rays[1, 5] == 1 and (np.delete(n_rays[1], 5) == 2).all()
        assert np.abs(np.delete(points[1] - c['truth'][1], 5, axis=0)).max() <= KNOWN_ANSWER_MM
        # one ray, no ray
        assert undetermined[2].all() and (n_rays[2] == 1).all() and undetermined[3].all() and (n_rays[3] == 0).all()
        # ... and a finite point at 0.5 degrees: the conditioning is 1 / sin(1 degree) = 57, so the bound scales by 57 / 3
        points, n_rays, _ = TR.expected(TR.determinacy_case(SPEC, weights, min_angle_deg=0.5), SPEC)
        assert np.isfinite(points[0]).all() and (n_rays[0] == 2).all()
        assert np.abs(points[0] - c['truth'][0]).max() <= KNOWN_ANSWER_MM * 57 / 3


def test_min_det_is_the_two_ray_determinant():
    """det A~ of two unit rays at angle t is sin^2 t / 4 (what min_angle_deg stands for)."""
    for deg in (0.5, 2.0, 30.0, 90.0, 170.0):
        t = np.radians(deg)
        d = np.array([[1.0, 0, 0], [np.cos(t), np.sin(t), 0]])
        a = (np.eye(3)[None] - d[:, :, None] * d[:, None, :]).sum(axis=0) / 2
        assert np.isclose(np.linalg.det(a), np.sin(t) ** 2 / 4, rtol=1e-12, atol=0)
        assert np.isclose(TR.min_det(deg), np.sin(t) ** 2 / 4, rtol=1e-15)
        assert np.isclose(MH.triangulation_min_det('uniform', min(deg, 90.0)), TR.min_det(min(deg, 90.0)), rtol=1e-15)


def _naive_groups(pi, fi, nv):
    groups = []
    for p in range(max(pi) + 1 if len(pi) else 0):
        boxes = [i for i in range(len(pi)) if pi[i] == p]
        if len({fi[i] for i in boxes}) < 2:
            boxes = []
        groups.append([i * nv + v for i in boxes for v in range(nv)])
    return groups


@pytest.mark.parametrize('pi,fi,nv', [
    ([0, 0, 0, 1, 1, 2, 2, 2, 2], [0, 1, 2, 0, 1, 0, 1, 2, 3], 1),        # ragged
    ([2, 0, 1, 0, 2, 1, 2], [0, 0, 0, 1, 1, 2, 2], 1),                     # unsorted
    ([3, 0, 3, 0, 5], [0, 0, 1, 1, 0], 1),                                 # gaps (1, 2, 4) and a person on one frame only (5)
    ([1, 0, 1, 0, 1], [0, 0, 1, 1, 1], 3),                                 # V > 1; person 1 twice on frame 1
    ([0, 0], [4, 4], 2),                                                   # two boxes, one frame: empty
    ([], [], 2),
], ids=['ragged', 'unsorted', 'gaps', 'views', 'one-frame', 'empty'])
def test_person_groups(pi, fi, nv):
    rows, starts = FR.person_groups(pi, fi, nv)
    want = _naive_groups(pi, fi, nv)
    assert rows.dtype == np.int32 and starts.dtype == np.int32 and len(starts) == len(want) + 1
    assert starts[0] == 0 and starts[-1] == len(rows)
    assert [list(rows[starts[p]:starts[p + 1]]) for p in range(len(want))] == want


def test_python_surface_checks_arguments_without_a_gpu():
    sig = inspect.signature(FR.triangulate_poses_in_frames)
    assert list(sig.parameters) == ['frames', 'boxes', 'model_path', 'cameras', 'person_index', 'frame_index', 'weights',
                                    'min_angle_deg', 'views', 'precision', 'check_finite', 'geometry', 'pixel_format',
                                    'color_matrix', 'crop_dtype']
    assert sig.parameters['weights'].default == 'covariance' and sig.parameters['min_angle_deg'].default == 2.0
    assert FR.WorldPoses._fields == ('poses', 'n_rays', 'residual', 'keypoints2d', 'joint_edges', 'joint_names')
    import metro_pose3d_amd
    assert metro_pose3d_amd.triangulate_poses_in_frames is FR.triangulate_poses_in_frames
    cams = TR.ring_cameras([0, 90])
    frames = [np.zeros((8, 8, 3), np.uint8)] * 2
    boxes = [[0, 0, 4, 4], [1, 1, 4, 4]]
    call = lambda cameras=cams, pi=(0, 0), fi=(0, 1), **kw: FR.triangulate_poses_in_frames(frames, boxes, 'no-such-model.npz',
                                                                                           cameras, pi, fi, **kw)
    with pytest.raises(ValueError, match='calibrated cameras'):
        call(cameras=None)
    with pytest.raises(ValueError, match='one Camera for several frames'):
        call(cameras=cams[0])
    with pytest.raises(ValueError, match='negative'):
        call(pi=(0, -1))
    with pytest.raises(ValueError, match='one value per box'):
        call(pi=(0, 0, 0))
    with pytest.raises(ValueError, match='one value per box'):
        call(fi=(0,))
    with pytest.raises(ValueError, match='frame_index must lie in'):
        call(fi=(0, 2))
    for bad in ('huber', None, 1):
        with pytest.raises(ValueError, match='weights must be'):
            call(weights=bad)
    for bad in (0, -1.0, 90.5, float('nan'), '2', True):
        with pytest.raises(ValueError, match='min_angle_deg'):
            call(min_angle_deg=bad)
    with pytest.raises(ValueError, match='negative'):
        FR.person_groups([0, -2], [0, 1])
    # heads.triangulate_joints: checked before the library or a device is touched
    m, nj = 4, SK.n_head
    c01, cov, places = torch.zeros((m, nj, 3)), torch.zeros((m, nj, 6)), torch.zeros(m * C.sizeof(_lib.MetroPlacement), dtype=torch.uint8)
    with pytest.raises(ValueError, match='weights must be'):
        MH.triangulate_joints(c01, cov, places, [0, 1], [0, 2], SPEC, weights='robust')
    with pytest.raises(ValueError, match='min_angle_deg'):
        MH.triangulate_joints(c01, cov, places, [0, 1], [0, 2], SPEC, min_angle_deg=0)
    with pytest.raises(ValueError, match='coords01 must be'):
        MH.triangulate_joints(c01[..., :2], cov, places, [0, 1], [0, 2], SPEC)
    with pytest.raises(ValueError, match='needs cov01'):
        MH.triangulate_joints(c01, None, places, [0, 1], [0, 2], SPEC)
    with pytest.raises(ValueError, match='needs cov01'):
        MH.triangulate_joints(c01, cov[:3], places, [0, 1], [0, 2], SPEC, weights='covariance')
    with pytest.raises(ValueError, match='MetroPlacement'):
        MH.triangulate_joints(c01, cov, places[:-1], [0, 1], [0, 2], SPEC)
    with pytest.raises(ValueError, match='starts'):
        MH.triangulate_joints(c01, None, places, [], [], SPEC, weights='uniform')


def test_new_symbol_in_header_bindings_and_library(lib):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'metro_hip.h')).read(), flags=re.S)
    name = 'metro_triangulate_joints'
    assert name in set(re.findall(r'\b(metro_[a-z0-9_]+)\s*\(', text)) and name in _lib.SIGNATURES and hasattr(lib, name)
    params = re.search(r'\b' + name + r'\s*\(([^)]*)\)', text).group(1)
    assert len(_lib.SIGNATURES[name][1]) == params.count(',') + 1 == 16
    assert re.search(r'#define\s+METRO_TRI_UNIFORM\s+0\b', text) and re.search(r'#define\s+METRO_TRI_COVARIANCE\s+1\b', text)
    assert (_lib.METRO_TRI_UNIFORM, _lib.METRO_TRI_COVARIANCE) == (0, 1)
    assert lib.metro_abi_version() == 8                    # the ABI is additive


def test_c_entry_rejects_bad_arguments(lib):
    """Every return below comes before any launch: no device is needed."""
    cs = SPEC.to_c(_lib.METRO_PREC_F16)
    p, md = C.c_void_p(256), TR.min_det(2.0)
    tri = lib.metro_triangulate_joints
    good = [p, p, p, 4, p, 4, p, 2, C.byref(cs), p, _lib.METRO_TRI_COVARIANCE, md, p, p, p, None]

    def call(**changes):
        a = list(good)
        for k, v in changes.items():
            a[int(k[1:])] = v
        return tri(*a)
    assert call(a8=None) == -1 and b'spec' in lib.metro_last_error()
    for w in (-1, 2):
        assert call(a10=w) == -1 and b'weights' in lib.metro_last_error()
    assert call(a7=-1) == -1 and b'negative' in lib.metro_last_error()
    assert call(a1=None) == -1 and b'cov01' in lib.metro_last_error()
    for k in (0, 2, 4):                                    # coords01, records, rows
        assert call(**{f'a{k}': None}) == -1 and b'group rows' in lib.metro_last_error()
    for k in (6, 9, 12, 13, 14):                           # starts, mirror, the three outputs
        assert call(**{f'a{k}': None}) == -1 and b'NULL' in lib.metro_last_error()
    # no persons: nothing to launch, whatever the pointers
    assert tri(None, None, None, 0, None, 0, None, 0, C.byref(cs), None, _lib.METRO_TRI_UNIFORM, md, None, None, None, None) == 0
    assert call(a7=0) == 0


# ---- the kernel's own per-joint code on the host -----------------------------------------------------------------------------

@pytest.fixture(scope='module')
def host_kernel(tmp_path_factory):
    """triangulate.hip's per-joint function is __host__ __device__: the source compiled for the host, one call per (person,
    output joint) where the launch has one thread."""
    tmp = tmp_path_factory.mktemp('host_triangulate')
    fn = compile_for_host(tmp, 'host_triangulate', ['triangulate.hip'], '''
extern "C" void host_triangulate_joints(const float* coords01, const float* cov01, const MetroPlacement* rec, int m, const int* rows,
                                        int n_rows, const int* starts, int n_persons, const MetroSpec* spec, const int* mirror,
                                        int weights, double min_det, float* points, int* n_rays, float* residual) {
    const metro::TriArgs a = metro::make_tri_args(coords01, cov01, rec, m, rows, n_rows, starts, n_persons, *spec, mirror, weights,
                                                  min_det, points, n_rays, residual);
    for (int idx = 0; idx < n_persons * spec->n_joints_out; ++idx) metro::triangulate_joint(a, idx);
}
''').host_triangulate_joints
    fn.restype = None
    fn.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(_lib.MetroSpec), C.c_void_p,
                                      C.c_int, C.c_double] + [C.c_void_p] * 3

    def run(c):
        n_persons, n_out = len(c['starts']) - 1, SK.n_out
        rec = np.ascontiguousarray(FR.pack_placements(c['places']))
        mirror = np.asarray(SK.out_mirror, np.int32)
        points = np.full((n_persons, n_out, 3), -7.0, np.float32)
        n_rays = np.full((n_persons, n_out), -7, np.int32)
        residual = np.full((n_persons, n_out), -7.0, np.float32)
        cs = SPEC.to_c(1)
        ptr = lambda a: C.c_void_p(a.ctypes.data)
        fn(ptr(c['coords01']), ptr(c['cov01']), ptr(rec), len(c['coords01']), ptr(c['rows']), len(c['rows']), ptr(c['starts']),
           n_persons, C.byref(cs), ptr(mirror), MH.TRI_WEIGHTS[c['weights']], TR.min_det(c['min_angle_deg']), ptr(points),
           ptr(n_rays), ptr(residual))
        return points, n_rays, residual
    return run


@pytest.mark.parametrize('name', list(CASES))
@pytest.mark.parametrize('weights', ['uniform', 'covariance'])
def test_kernel_code_on_the_host_matches_the_restatement(host_kernel, name, weights):
    c = CASES[name](SPEC, weights)
    want = TR.expected(c, SPEC)
    got = host_kernel(c)
    worst = TR.compare(got, want, PARITY_MM)
    print(f'{name}, {weights}: worst point {worst[0]:.2e} mm, worst residual {worst[1]:.2e} mm')
    TR.check_case(name, c, got, KNOWN_ANSWER_MM)
