"""Per-joint heat-map covariance and peak, without a GPU: the fp64 restatement the GPU tests compare against
(tests/heat_moments_ref.py) on known answers and against the oracle's soft-argmax, the new C symbols in header, bindings and
library, and the argument checks of the Python surface that run before any device is touched."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from metro_pose3d_amd import ModelSpec, _lib
from tests import heat_moments_ref as HM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('metro_moments_scratch_bytes', 'metro_forward_moments', 'metro_head_f16_moments', 'metro_softargmax01_moments',
               'metro_place_covariances')
S, D, J = 6, 4, 3


def _volume(fill=-1e4):
    return np.full((1, S, S, D * J), fill, np.float64)


def test_one_hot_volume_has_no_spread():
    lg = _volume()
    for j, (y, x, d) in enumerate([(0, 0, 0), (2, 5, 1), (S - 1, S - 1, D - 1)]):
        lg[0, y, x, d * J + j] = 0.0
    mu, cov, peak, _ = HM.moments(lg, J, D)
    assert (cov == 0).all() and (peak == 1).all()
    assert np.allclose(mu[0, 1], [HM.lin01(S)[5], HM.lin01(S)[2], HM.lin01(D)[1]], rtol=0, atol=1e-15)


def test_uniform_volume_has_the_variance_of_a_linspace():
    mu, cov, peak, _ = HM.moments(_volume(0.0), J, D)
    var = lambda k: (k + 1) / (12.0 * (k - 1))           # variance of linspace(0, 1, k) under equal weights
    for a, k in ((0, S), (1, S), (2, D)):
        assert np.allclose(cov[..., a, a], var(k), rtol=1e-6)          # 1e-6: the coordinates are fp32 values
    off = cov[..., [0, 0, 1], [1, 2, 2]]
    assert np.abs(off).max() < 1e-9
    assert np.allclose(peak, 1.0 / (S * S * D), rtol=1e-12) and np.allclose(mu, 0.5, atol=1e-7)


def test_two_voxel_mixture_has_the_known_cross_term():
    lg = _volume()
    w = 0.25                                               # p = (w, 1 - w) on voxels a and b of joint 0
    lg[0, 1, 0, 0 * J + 0] = np.log(w)
    lg[0, 4, 3, 2 * J + 0] = np.log(1 - w)
    mu, cov, peak, _ = HM.moments(lg[..., :], J, D)
    xs, zs = HM.lin01(S), HM.lin01(D)
    a, b = np.array([xs[0], xs[1], zs[0]]), np.array([xs[3], xs[4], zs[2]])
    d = b - a
    assert np.allclose(cov[0, 0], w * (1 - w) * np.outer(d, d), rtol=1e-12, atol=1e-15)
    assert np.isclose(cov[0, 0, 0, 1], w * (1 - w) * d[0] * d[1]) and cov[0, 0, 0, 1] > 0
    assert np.isclose(peak[0, 0], 1 - w) and np.allclose(mu[0, 0], w * a + (1 - w) * b)


def test_mean_is_the_oracle_soft_argmax():
    rng = np.random.default_rng(5)
    lg = rng.standard_normal((2, S, S, D * J)) * 3.0
    mu, cov, peak, oracle_mu = HM.moments(lg, J, D)
    assert np.allclose(mu, oracle_mu, rtol=0, atol=1e-14)
    ev = np.linalg.eigvalsh(cov)
    assert (ev > 0).all() and (peak > 1.0 / (S * S * D)).all() and (peak < 1).all()
    assert np.array_equal(HM.cov6(cov)[..., 3], cov[..., 0, 1])


def test_new_symbols_in_header_bindings_and_library(lib):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'metro_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(metro_[a-z0-9_]+)\s*\(', text))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    # argument counts of the bindings equal the header's parameter lists
    for name in NEW_SYMBOLS:
        params = re.search(r'\b' + name + r'\s*\(([^)]*)\)', text).group(1)
        assert len(_lib.SIGNATURES[name][1]) == params.count(',') + 1, name


def test_scratch_size_and_c_argument_checks(lib):
    spec = ModelSpec(50, 16, 'h36m')
    cs = spec.to_c(_lib.METRO_PREC_F16)
    side, nj = spec.heatmap_side, spec.skeleton.n_head
    assert lib.metro_moments_scratch_bytes(C.byref(cs), 3) == 3 * (side * side // 32) * nj * 6 * 8
    assert lib.metro_moments_scratch_bytes(C.byref(cs), 0) == -1 and lib.metro_moments_scratch_bytes(None, 3) == -1
    p = C.c_void_p(256)
    st = lib.metro_place_covariances(p, p, None, 2, 1, C.byref(cs), None, _lib.METRO_COORDS_CAMERA, p, p, None)
    assert st == -1 and b'records' in lib.metro_last_error()
    st = lib.metro_place_covariances(p, p, None, 2, 0, C.byref(cs), None, _lib.METRO_COORDS_CROP, p, p, None)
    assert st == -1 and b'views' in lib.metro_last_error()
    st = lib.metro_softargmax01_moments(p, 1, C.byref(cs), 0, p, None, p, p, p, None)
    assert st == -1
    plan = C.c_void_p()
    assert lib.metro_plan_create(C.byref(cs), 4, C.byref(plan)) == 0
    try:
        # cov01 without peak / scratch; uint8 crops on a misaligned pointer
        assert lib.metro_forward_moments(plan, p, 0, 1, p, None, p, None, None, p, None) == -1
        assert b'go together' in lib.metro_last_error()
        assert lib.metro_forward_moments(plan, C.c_void_p(257), 1, 1, p, None, None, None, None, p, None) == -1
        assert b'aligned' in lib.metro_last_error()
    finally:
        lib.metro_plan_destroy(plan)


def test_default_dispatch_is_unchanged_and_moments_have_their_own_ids():
    """A plan's layer kernels (metro_plan_layer_kernel: the default forward) carry no moments instantiation."""
    from metro_pose3d_amd.engine import Engine
    eng = Engine(ModelSpec(50, 16, 'h36m'), None, 'f16', max_batch=64)
    ids = eng.layer_kernels(64)
    assert not any('moments' in k for k in ids) and ids[-1] == 'softargmax_finalize<acc32>', ids[-2:]
    eng.close()


def test_python_surface_checks_arguments_without_a_gpu():
    from metro_pose3d_amd import heads as MH, inference as INF, frames as FR
    from metro_pose3d_amd.engine import Engine
    spec = ModelSpec(50, 16, 'h36m')
    for fn, name in ((INF.estimate_pose, 'return_uncertainty'), (FR.estimate_pose_in_frames, 'return_uncertainty'),
                     (FR.locate_poses_in_frames, 'return_uncertainty'), (Engine.forward, 'cov01'), (Engine.forward, 'peak')):
        assert name in inspect.signature(fn).parameters, (fn.__name__, name)
        assert inspect.signature(fn).parameters[name].default in (False, None)
    assert FR.FramePoses._fields[-2:] == ('covariance', 'peak') and FR.FramePoses._field_defaults == {'covariance': None, 'peak': None}
    assert INF.PoseUncertainty._fields == ('covariance', 'peak')
    with pytest.raises(ValueError, match='logits must be'):
        MH.moments_from_logits(torch.zeros((1, 4, 4, 8)), spec)
    with pytest.raises(ValueError, match='precise'):
        MH.moments_from_logits(torch.zeros((1, 16, 16, spec.n_head_channels)), spec, precise=3)
    nj = spec.skeleton.n_head
    cov, peak = torch.zeros((4, nj, 6)), torch.zeros((4, nj))
    with pytest.raises(ValueError, match='coords'):
        MH.place_covariances(cov, peak, spec, coords='frame')
    with pytest.raises(ValueError, match='cov01 must be'):
        MH.place_covariances(cov[..., :5], peak, spec)
    with pytest.raises(ValueError, match='views'):
        MH.place_covariances(cov, peak, spec, n_views=3)
    with pytest.raises(ValueError, match='records'):
        MH.place_covariances(cov, peak, spec, coords='camera')
    sym = MH.cov6_to_3x3(torch.arange(6.0))
    assert torch.equal(sym, sym.T) and sym[0, 1] == 3 and sym[0, 2] == 4 and sym[1, 2] == 5 and sym[2, 2] == 2
    # the CLI knows the flag
    with pytest.raises(SystemExit):
        INF.main(['--uncertainty'])                        # --model-path is still required: argparse exits, not "unknown flag"
    eng = Engine(spec, None, 'f16', max_batch=4)
    eng._blob, eng.device = object(), torch.device('cpu')          # past the "no parameters" check, never launched
    x = torch.zeros((2, 256, 256, 3))
    with pytest.raises(ValueError, match='go together'):
        eng.forward(x, cov01=torch.zeros((2, nj, 6)))
    with pytest.raises(ValueError, match='cov01 must be'):
        eng.forward(x, cov01=torch.zeros((2, nj, 5)), peak=torch.zeros((2, nj)))
    with pytest.raises(ValueError, match='peak must be'):
        eng.forward(x, cov01=torch.zeros((2, nj, 6)), peak=torch.zeros((2, nj), dtype=torch.float64))
    eng._blob = None
    eng.close()
