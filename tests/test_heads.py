"""Alternative decode heads.  CPU part: the oracle (reference code restated with
NumPy + the reference's own scipy call) against the independent lmder restatement and analytical known answers.
GPU part: the HIP path through the C ABI against the oracle."""
import numpy as np
import pytest
import scipy.optimize

from metro_pose3d_amd import ModelSpec
from oracle import heads as OH
from oracle.lm1 import lmder1
from oracle.spec import head_joint_info
from tests import helpers as H


def _problem(rng, spec, n):
    return H.consistent_problem(rng, spec, n)


def _lm1(c, d, e, target, stats=None):
    """oracle/lm1.py on the reference's residual and (inexact) Jacobian -> (z, info, nfev)."""
    c, d, e = (np.asarray(v, np.float64) for v in (c, d, e))
    with np.errstate(invalid='ignore', divide='ignore'):
        rec = lambda z: np.sqrt(z ** 2 * c + z * d + e)
        return lmder1(lambda z: rec(np.float64(z)) - target, lambda z: (np.float64(z) * c + d) / rec(np.float64(z)), 2000.0,
                      stats=stats)[:3]


def test_lmder_restatement_matches_scipy():
    """oracle/lm1.py follows MINPACK's control flow: same x as scipy.optimize.least_squares(method='lm') on the
    reference's residual / (inexact) Jacobian, to fp64 rounding, on 300 random poses."""
    rng = np.random.default_rng(0)
    spec = ModelSpec(50, 16, 'h36m')
    ji, p, c01, inv_k, bones = _problem(rng, spec, 300)
    cam, dz = OH.camcoords_and_delta_z(c01, inv_k, spec.stride)
    target = bones.mean(axis=0) * 1.03
    worst = 0.0
    for i in range(300):
        x, d_z = cam[i], dz[i]
        a = np.asarray([x[u] - x[v] for u, v in ji.edges]); y = x * d_z[:, None]
        b = np.asarray([y[u] - y[v] for u, v in ji.edges])
        c, d, e = np.sum(a ** 2, axis=1), np.sum(2 * a * b, axis=1), np.sum(b ** 2, axis=1)
        rec = lambda z: np.sqrt(z ** 2 * c + z * d + e)
        ref = OH.optimize_z_offset_by_bones_single(x, d_z, target, ji.edges)
        mine, info, nfev, _ = lmder1(lambda z: rec(np.float64(z)) - target, lambda z: (np.float64(z) * c + d) / rec(np.float64(z)), 2000.0)
        assert 1 <= info <= 4 and nfev < 100
        worst = max(worst, abs(mine - ref))
    assert worst <= 1e-9, worst


def test_lmder_restatement_matches_scipy_on_the_hard_corpus():
    """The corpus the device solve is tested on (tests/helpers.py bone_case: three skeletons x friendly / noisy / mis-scaled /
    collapsed x shared / per-pose targets, 130 problems each): oracle/lm1.py gives scipy's z to 1e-9 on every problem, and
    the corpus is hard -- MINPACK's exit codes 1, 2, 3, 4 and 5 (maxfev) are all reached, and so are both Givens rotations
    of qrsolv and more than one pass of lmpar's loop.  A generator that stopped producing such problems fails here, before
    any GPU run.  No problem needs excluding: scipy's answer moves by less than max(1 mm, one float32 spacing of itself)
    when the fp32 coefficients move by an ulp (the cap the GPU tests assert is 2 % per family)."""
    import collections
    codes, stats, worst, longest = collections.Counter(), {}, 0.0, 0
    for dataset in ('h36m', 'many19', 'merged'):
        for family in H.BONE_FAMILIES:
            for per_pose in (False, True):
                case = H.bone_case(dataset, family, per_pose)
                assert (~case.held).mean() <= 0.02, (dataset, family, per_pose, (~case.held).sum())
                for i in range(case.n):
                    cde = OH.edge_coefficients(case.cam[i], case.dz[i], case.ji.edges)
                    z, info, nfev = _lm1(*cde, case.targets[i] if per_pose else case.targets, stats)
                    codes[info] += 1
                    longest = max(longest, nfev)
                    assert np.isfinite(case.z[i]) and abs(z - case.z[i]) <= 1e-9, (dataset, family, per_pose, i, z, case.z[i])
                    worst = max(worst, abs(z - case.z[i]))
    print(f'exit codes {dict(sorted(codes.items()))}, longest solve {longest} evaluations, branches {stats}, worst |dz| {worst:.1e}')
    assert all(codes[k] > 0 for k in (1, 2, 3, 4, 5)), codes
    assert longest >= 100
    assert stats.get('givens_cotan', 0) > 0 and stats.get('givens_tan', 0) > 0, stats
    assert stats['lmpar_iterations'] == stats['givens_cotan'] + stats['givens_tan']


def test_the_reference_jacobian_is_not_the_derivative():
    """Teeth of the corpus: the reference's Jacobian is (z c + d) / len; with the true derivative (z c + d/2) / len scipy
    stops elsewhere, by far more than the tolerance the device is held to, on most of the noisy problems -- a device
    solver 'corrected' to the derivative could not pass."""
    case = H.bone_case('merged', 'noisy', True)
    off = np.empty(case.n)
    for i in range(case.n):
        cde = OH.edge_coefficients(case.cam[i], case.dz[i], case.ji.edges)
        off[i] = abs(OH.z_offset_from_coefficients(*cde, case.targets[i], half_d_jacobian=True) - case.z[i])
    print(f'median |dz| with the true derivative: {np.median(off):.3g} mm, {np.median(off / case.tol):.3g} tolerances')
    assert (off > 10 * case.tol).mean() > 0.5, np.median(off / case.tol)


def test_bone_length_head_known_answers():
    """KA: exact per-pose bone lengths and noise-free delta_z -> the solve recovers the root depth, back_project
    the pose (to fp32 rounding of the rays); true-root-depth reproduces it by construction."""
    rng = np.random.default_rng(1)
    spec = ModelSpec(50, 16, 'h36m')
    ji, p, c01, inv_k, bones = _problem(rng, spec, 8)
    c01[..., 2] = ((p[..., 2] - p[:, -1:, 2]) / 2200.0 + 0.5).astype(np.float32)      # no depth noise
    out, z = OH.backproject_bone_lengths(c01, inv_k, bones, ji.edges, spec.stride)
    assert np.abs(z - p[:, -1, 2]).max() < 2.0                       # mm; fp32 rays at ~4 m
    assert np.abs(out - p).max() < 3.0
    out2 = OH.backproject_root_depth(c01, inv_k, p[:, -1, 2], spec.stride)
    assert np.abs(out2 - p).max() < 1.0


def test_to_orig_cam_mirrors_on_negative_determinant():
    ji = head_joint_info('h36m')
    rng = np.random.default_rng(2)
    x = rng.normal(0, 500, (2, ji.n_joints, 3)).astype(np.float32)
    rot = np.stack([np.eye(3), np.diag([-1.0, 1.0, 1.0])]).astype(np.float32)
    y = OH.to_orig_cam(x, rot, ji.mirror_mapping)
    assert np.array_equal(y[0], x[0])
    flipped = x[1] * np.array([-1, 1, 1], np.float32)
    assert np.array_equal(y[1], flipped[ji.mirror_mapping])
    assert ji.names[ji.mirror_mapping[ji.names.index('lwri')]] == 'rwri' and ji.mirror_mapping[ji.names.index('neck')] == ji.names.index('neck')


def test_skeleton_tables_agree_with_oracle():
    for ds in ('h36m', 'merged', 'many19'):
        sk = ModelSpec(50, 16, ds).skeleton
        ji = head_joint_info(ds)
        assert list(sk.head_mirror) == ji.mirror_mapping
        assert [tuple(e) for e in sk.head_edges] == [tuple(e) for e in ji.edges]


# ---------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize('spec', [ModelSpec(50, 16, 'h36m'), ModelSpec(50, 8, 'many19'), ModelSpec(50, 32, 'h36m', centered_stride=False),
                                  ModelSpec(50, 16, 'h36m', proc_side=384), ModelSpec(50, 32, 'many19', proc_side=224, centered_stride=False)],
                         ids=['h36m-s16', 'many19-s8', 'h36m-s32-nc', 'h36m-s16-side384', 'many19-s32-nc-side224'])
def test_gpu_bone_length_head(cuda, spec):
    import torch
    from metro_pose3d_amd import heads as MH
    rng = np.random.default_rng(spec.stride)
    n = 130                                                          # > one 64-thread block of poses
    ji, p, c01, inv_k, bones = _problem(rng, spec, n)
    target = bones.mean(axis=0) * 0.97
    ref, zref = OH.backproject_bone_lengths(c01, inv_k, target, ji.edges, spec.stride, spec.proc_side, spec.centered_stride)
    got, z = MH.backproject_bone_lengths(torch.from_numpy(c01).to(cuda), inv_k, target, spec)
    got, z = got.cpu().numpy(), z.cpu().numpy()
    assert np.abs(z - zref).max() <= 1e-3, np.abs(z - zref).max()             # mm (fp32 z_offset at ~4000 mm: ulp 2.4e-4)
    assert np.abs(got - ref).max() <= 1e-3 * 4, np.abs(got - ref).max()
    # per-pose targets ('bone-lengths-true'), root-relative + export permutation
    ref2, _ = OH.backproject_bone_lengths(c01, inv_k, bones, ji.edges, spec.stride, spec.proc_side, spec.centered_stride)
    ref2 = OH.root_relative(ref2)[:, list(spec.skeleton.permutation)]
    got2, _ = MH.backproject_bone_lengths(torch.from_numpy(c01).to(cuda), inv_k, bones, spec, root_relative=True, permute=True)
    assert got2.shape == (n, spec.skeleton.n_out, 3)
    assert np.abs(got2.cpu().numpy() - ref2).max() <= 4e-3
    # true-root-depth
    ref3 = OH.backproject_root_depth(c01, inv_k, p[:, -1, 2], spec.stride, spec.proc_side, spec.centered_stride)
    got3 = MH.backproject_root_depth(torch.from_numpy(c01).to(cuda), inv_k, p[:, -1, 2], spec).cpu().numpy()
    assert np.abs(got3 - ref3).max() <= 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize('family', H.BONE_FAMILIES)
@pytest.mark.parametrize('dataset', ['h36m', 'many19', 'merged'])
def test_gpu_bone_length_head_on_the_hard_corpus(cuda, dataset, family):
    """metro_backproject_bone_lengths on the corpus of test_lmder_restatement_matches_scipy_on_the_hard_corpus (130 poses: more
    than two 64-lane blocks; `merged` fills 53 of the 64 per-lane joint slots), shared and per-pose targets, against
    oracle/heads.py (scipy).
    Tolerance on z (tests/helpers.py BoneCase): max(1e-3 mm, k ulp32(|z|)), k = 1 + 4 m / ulp32(|z|) per problem, where m is
    how far scipy's own answer moves when the oracle's fp32 coefficients c, d, e move by one ulp (all up, all down, two
    random sign patterns), 4 the factor for summation order, and the 1 the final cast to fp32 of a value that may sit on
    a rounding boundary.  Largest k in the corpus: 553 (mis-scaled, per-pose targets: 0.03 mm at z = 113 m); the collapsed
    family's offsets are ~1e7 mm (ulp32 1 to 2 mm), k <= 4.4.  No problem is excluded (cap 2 %).
    Measured on the MI355X: worst |z - scipy's| 0 mm in every family (bit-equal after the cast to fp32), poses bit-equal.
    No NaN where scipy is finite; poses (head order and exported order, root-relative) within 2 tol_z + 1e-6 of the pose."""
    import torch
    from metro_pose3d_amd import heads as MH
    for per_pose in (False, True):
        case = H.bone_case(dataset, family, per_pose)
        spec, what = case.spec, f'{dataset} {family} {"per-pose" if per_pose else "shared"}'
        c01 = torch.from_numpy(case.c01).to(cuda)
        got, z = MH.backproject_bone_lengths(c01, case.inv_k, case.targets, spec)
        case.check_z(z.cpu().numpy(), what)
        ref = OH.back_project(case.cam, case.dz, case.z32)
        case.check_poses(got.cpu().numpy(), ref, what)
        got2, z2 = MH.backproject_bone_lengths(c01, case.inv_k, case.targets, spec, root_relative=True, permute=True)
        assert got2.shape == (case.n, spec.skeleton.n_out, 3) and torch.equal(z2, z)
        case.check_poses(got2.cpu().numpy(), OH.root_relative(ref)[:, list(spec.skeleton.permutation)], what + ' exported')


@pytest.mark.gpu
def test_gpu_coords01_and_to_orig_cam(cuda):
    import torch
    from metro_pose3d_amd import heads as MH
    from oracle.forward import soft_argmax01
    spec = ModelSpec(50, 16, 'h36m')
    rng = np.random.default_rng(5)
    logits = (rng.standard_normal((5, 16, 16, spec.n_head_channels)) * 4).astype(np.float32)
    got = MH.coords01_from_logits(torch.from_numpy(logits).to(cuda), spec, precise=1).cpu().numpy()
    ref = soft_argmax01(torch.from_numpy(logits).permute(0, 3, 1, 2).double(), spec.skeleton.n_head, spec.depth)[1].numpy()
    assert got.shape == ref.shape == (5, 17, 3)
    assert np.abs(got - ref).max() <= 1e-6
    c01 = rng.uniform(0, 1, (7, 17, 3)).astype(np.float32)
    assert np.array_equal(MH.heatmap_to_25d(torch.from_numpy(c01).to(cuda), spec).cpu().numpy(), OH.heatmap_to_25d(c01, spec.stride))
    # the last image pixel (and so the scale of a heat-map coordinate) follows the model's crop side
    for sp in (ModelSpec(50, 16, 'h36m', proc_side=384), ModelSpec(50, 32, 'h36m', proc_side=224, centered_stride=False),
               ModelSpec(50, 8, 'h36m', proc_side=320)):
        got25 = MH.heatmap_to_25d(torch.from_numpy(c01).to(cuda), sp).cpu().numpy()
        assert np.array_equal(got25, OH.heatmap_to_25d(c01, sp.stride, sp.proc_side, sp.centered_stride)), sp
        assert not np.array_equal(got25, OH.heatmap_to_25d(c01, sp.stride, 256, sp.centered_stride))
    # an 18 x 18 heat map (crop side 288): 324 pixels, not whole 32-pixel slabs
    sp = ModelSpec(50, 16, 'h36m', proc_side=288)
    lg = (rng.standard_normal((3, 18, 18, sp.n_head_channels)) * 4).astype(np.float32)
    got = MH.coords01_from_logits(torch.from_numpy(lg).to(cuda), sp, precise=1).cpu().numpy()
    ref = soft_argmax01(torch.from_numpy(lg).permute(0, 3, 1, 2).double(), sp.skeleton.n_head, sp.depth)[1].numpy()
    assert np.abs(got - ref).max() <= 1e-6
    ji = head_joint_info('h36m')
    x = rng.normal(0, 500, (6, 17, 3)).astype(np.float32)
    q, _ = np.linalg.qr(rng.normal(size=(6, 3, 3)))
    q[::2] *= np.sign(np.linalg.det(q[::2]))[:, None, None]                    # proper rotations
    q[1::2] *= -np.sign(np.linalg.det(q[1::2]))[:, None, None]                 # reflections
    rot = q.astype(np.float32)
    got = MH.to_orig_cam(torch.from_numpy(x).to(cuda), rot, ji.mirror_mapping).cpu().numpy()
    ref = OH.to_orig_cam(x, rot, ji.mirror_mapping)
    assert np.abs(got - ref).max() <= 1e-3


@pytest.mark.gpu
def test_gpu_head_argument_errors(cuda):
    import torch
    from metro_pose3d_amd import heads as MH
    spec = ModelSpec(50, 16, 'h36m')
    c = torch.zeros((2, 17, 3), device=cuda)
    with pytest.raises(ValueError):
        MH.backproject_bone_lengths(c, np.zeros((2, 3, 3)), np.ones(5), spec)            # wrong number of bones
    with pytest.raises(ValueError):
        MH.backproject_bone_lengths(c[:, :5], np.zeros((2, 3, 3)), np.ones(16), spec)    # wrong joint count
    with pytest.raises(ValueError):
        MH.to_orig_cam(c, np.zeros((2, 3, 3)), [0, 1, 2])


def test_more_than_64_joints_or_edges_are_refused_before_any_launch(lib):
    """The per-lane arrays of backproject_kernel and place_poses_kernel hold HEAD_MAX = METRO_MAX_JOINTS = 64 joints / edges:
    65 are an argument error from the C ABI, and nothing is launched (dry-run notes record no kernel; without a GPU a launch
    would be a HIP error, not METRO_ERR_INVALID_ARG)."""
    import ctypes as C
    from metro_pose3d_amd import _lib
    p = C.c_void_p(4096)                                   # any non-NULL pointer: nothing may read it
    good = ModelSpec(50, 16, 'merged').to_c(1)
    lib.metro_kernel_notes(2)
    try:
        for field in ('n_joints_head', 'n_joints_out', 'edges'):
            cs = ModelSpec(50, 16, 'merged').to_c(1)
            ne = 18
            if field == 'edges':
                ne = _lib.METRO_MAX_JOINTS + 1
            else:
                setattr(cs, field, _lib.METRO_MAX_JOINTS + 1)
            st = lib.metro_backproject_bone_lengths(p, p, p, 0, p, ne, 3, C.byref(cs), 0, 0, p, p, None)
            assert st == -1 and lib.metro_last_kernel_id() == b'', (field, st, lib.metro_last_error())
            assert (b'edges' if field == 'edges' else b'joint counts') in lib.metro_last_error()
            st = lib.metro_place_poses(p, p, p, 3, C.byref(cs), _lib.METRO_SCALE_BONE_LENGTHS, p, 0, None, p, ne, p,
                                       _lib.METRO_COORDS_CAMERA, p, p, p, None)
            assert st == -1 and lib.metro_last_kernel_id() == b'', (field, st, lib.metro_last_error())
            if field != 'edges':
                assert lib.metro_backproject_root_depth(p, p, p, 3, C.byref(cs), 0, 0, p, None) == -1
                assert lib.metro_heatmap_to_25d(p, 3, C.byref(cs), p, None) == -1
        # 64 edges on 53 joints pass the check: the dry run records the kernel it would have launched
        st = lib.metro_place_poses(p, p, p, 3, C.byref(good), _lib.METRO_SCALE_BONE_LENGTHS, p, 0, None, p, _lib.METRO_MAX_JOINTS, p,
                                   _lib.METRO_COORDS_CAMERA, p, p, p, None)
        assert st == 0 and lib.metro_last_kernel_id() == b'place_poses', (st, lib.metro_last_error(), lib.metro_last_kernel_id())
    finally:
        lib.metro_kernel_notes(0)
