"""metro_place_poses, metro_forward_coords01 and locate_poses_in_frames on the MI355X: the placement launch against the
reference's outputs (tests/golden/ref_placement_v1.npz), bit equality with the existing head kernels, the forward's coords01
against metro_forward / metro_softargmax01, and the whole call against the oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

from metro_pose3d_amd import ModelSpec, _lib
from metro_pose3d_amd._lib import check
from metro_pose3d_amd.frames import SCALE_RECOVERY, COORDS, pack_placements
from tests import oracle_placement as OPL
from tests.test_placement import fixture_params

pytestmark = pytest.mark.gpu

SPEC = ModelSpec(50, 32, 'h36m')             # the fixture's constants: stride 32, 256 px crops, 2200 mm box, centred
SK = SPEC.skeleton


def _dev(a, cuda, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))).to(cuda)


def _place(cuda, spec, coords01, params, scale, coords, poses=None, bones=None, root=None):
    """One metro_place_poses launch -> (poses [n, Jout, 3], keypoints [n, Jout, 2], z_offset [n]) as host arrays."""
    sk = spec.skeleton
    n = len(coords01)
    c01 = _dev(coords01, cuda, np.float32)
    rel = _dev(poses, cuda, np.float32) if poses is not None else None
    recs = _dev(pack_placements(params), cuda)
    t = _dev(bones, cuda, np.float64) if bones is not None else None
    rz = _dev(root, cuda, np.float32) if root is not None else None
    edges = _dev(np.asarray(sk.head_edges, np.int32), cuda)
    mirror = _dev(np.asarray(sk.out_mirror, np.int32), cuda)
    out = torch.full((n, sk.n_out, 3), 12345.0, device=cuda)
    kp = torch.full((n, sk.n_out, 2), 12345.0, device=cuda)
    z = torch.full((n,), 12345.0, device=cuda)
    p = lambda x: C.c_void_p(x.data_ptr() if x is not None else 0)
    cs = spec.to_c(0)
    check(_lib.load().metro_place_poses(p(c01), p(rel), p(recs), n, C.byref(cs), SCALE_RECOVERY[scale], p(t),
                                        int(t is not None and t.dim() == 2), p(rz), p(edges), len(sk.head_edges), p(mirror),
                                        COORDS[coords], p(out), p(kp), p(z), C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)),
          'metro_place_poses')
    return out.cpu().numpy(), kp.cpu().numpy(), z.cpu().numpy()


@pytest.mark.parametrize('scale', OPL.SCALES)
def test_place_poses_matches_the_reference(cuda, scale):
    """3 cameras x 3 scale recoveries x 3 coordinate frames against the reference's outputs.
    Bounds (fp32 derivation): the kernel evaluates the reference's fp32 formulas; what can differ is (a) K^-1, whose entries
    agree with the reference's to a few ulp (our look_at_box, tests/test_frames.py: rtol 1e-6 on K), (b) the einsum's summation
    order (1 ulp per ray component), (c) the z offset, whose fp64 solve on fp32 coefficients carries (a)-(b) through the bone
    fit.  A 3D point is a ray times a depth of 3-6 m: 3-4 fp32 roundings of 6e-8 -> ~3e-7 relative, so the issue's 1e-4 is
    loose; measured on the MI355X: 0 (every value bit-equal to the reference's), bound 1e-6 relative.  Keypoints: the
    reference's general branch in fp32 (at camera_depth 4000 mm) vs our fp32 ray through the rounded rotation: ~1e-7 relative
    of a 1000-2000 px focal length, 1e-4..1e-3 px; measured 2.4e-4 px, bound 1e-3 px (the issue's 1e-2 tightened)."""
    d, q = fixture_params()
    perm = list(SK.permutation)
    key = scale.replace('-', '_')
    worst3, worstkp = 0.0, 0.0
    for coords in OPL.COORDS:
        got, kp, z = _place(cuda, SPEC, d['coords01'], q, scale, coords, poses=d['metro_crop'][:, perm],
                            bones=d['bone_targets'] if scale == 'bone-lengths' else None,
                            root=d['root_depth'] if scale == 'true-root-depth' else None)
        want = d[f'{key}_{coords}'][:, perm]
        rel = np.abs(got - want).max() / np.abs(want).max()
        worst3 = max(worst3, rel)
        assert rel <= 1e-6, (coords, rel)
        if scale != 'metro':
            assert np.abs(z - d[f'{key}_z_offset']).max() <= 1e-6 * np.abs(d[f'{key}_z_offset']).max()
        worstkp = max(worstkp, np.abs(kp - d['keypoints'][:, perm]).max())
        assert worstkp <= 1e-3, (coords, worstkp)
    print(f'{scale}: worst 3D relative error {worst3:.2e}, worst keypoint error {worstkp:.2e} px')


def test_place_poses_is_bit_identical_to_the_head_kernels(cuda):
    from metro_pose3d_amd import heads as MH
    d, q = fixture_params()
    got, _, z = _place(cuda, SPEC, d['coords01'], q, 'bone-lengths', 'crop', bones=d['bone_targets'])
    ref, zref = MH.backproject_bone_lengths(_dev(d['coords01'], cuda), q.inv_intrinsics, d['bone_targets'], SPEC,
                                            root_relative=False, permute=True)
    assert np.array_equal(got, ref.cpu().numpy()) and np.array_equal(z, zref.cpu().numpy())
    shared = d['bone_targets'].mean(axis=0)
    got, _, z = _place(cuda, SPEC, d['coords01'], q, 'bone-lengths', 'crop', bones=shared)
    ref, zref = MH.backproject_bone_lengths(_dev(d['coords01'], cuda), q.inv_intrinsics, shared, SPEC, permute=True)
    assert np.array_equal(got, ref.cpu().numpy()) and np.array_equal(z, zref.cpu().numpy())
    rel = d['metro_crop'][:, list(SK.permutation)]
    for coords, rot in (('camera', q.rot_to_orig_cam), ('world', q.rot_to_world)):
        got, _, _ = _place(cuda, SPEC, d['coords01'], q, 'metro', coords, poses=rel)
        ref = MH.to_orig_cam(_dev(rel, cuda), rot, SK.out_mirror).cpu().numpy()
        assert np.array_equal(got, ref), coords
    # a reflection (det < 0) mirrors the joints in both kernels alike
    q2 = q._replace(rot_to_orig_cam=-q.rot_to_orig_cam)
    got, _, _ = _place(cuda, SPEC, d['coords01'], q2, 'metro', 'camera', poses=rel)
    assert np.array_equal(got, MH.to_orig_cam(_dev(rel, cuda), q2.rot_to_orig_cam, SK.out_mirror).cpu().numpy())
    # absolute modes, proper and improper rotations (half the crops reflected): back-projection of the mirror joint equals
    # metro_backproject_bone_lengths followed by metro_to_orig_cam (+ cam_loc for world)
    sign = np.where(np.arange(len(q.rot_to_orig_cam)) % 2, -1, 1).astype(np.float32)[:, None, None]
    q3 = q._replace(rot_to_orig_cam=q.rot_to_orig_cam * sign, rot_to_world=q.rot_to_world * sign)
    assert (np.linalg.det(q3.rot_to_orig_cam[1::2].astype(np.float64)) < 0).all()
    crop, _ = MH.backproject_bone_lengths(_dev(d['coords01'], cuda), q.inv_intrinsics, d['bone_targets'], SPEC,
                                          root_relative=False, permute=True)
    for coords, rot in (('camera', q3.rot_to_orig_cam), ('world', q3.rot_to_world)):
        got, _, _ = _place(cuda, SPEC, d['coords01'], q3, 'bone-lengths', coords, bones=d['bone_targets'])
        ref = MH.to_orig_cam(crop, rot, SK.out_mirror).cpu().numpy()
        if coords == 'world':
            ref = ref + q3.cam_loc[:, None]
        assert np.array_equal(got, ref), coords


def test_keypoints_behind_the_camera_are_nan(cuda):
    d, q = fixture_params()
    q = q._replace(homography=q.homography.copy(), rot_to_orig_cam=q.rot_to_orig_cam.copy())
    q.homography[19] = np.diag([1., 1., -1.]).astype(np.float32)          # undistorted camera: w < 0
    q.rot_to_orig_cam[0] = np.diag([1., -1., -1.]).astype(np.float32)     # distorted camera: z < 0 (a proper rotation)
    _, kp, _ = _place(cuda, SPEC, d['coords01'], q, 'metro', 'crop', poses=d['metro_crop'][:, list(SK.permutation)])
    assert np.isnan(kp[19]).all() and np.isnan(kp[0]).all() and np.isfinite(kp[1:19]).all()


def _toy_engine_model(tmp_path, proc_side=256):
    from metro_pose3d_amd import save_model, synth
    spec = ModelSpec(50, 32, 'h36m', base_width=8, proc_side=proc_side)
    params = synth.make_params(50, spec.n_head_channels, 8, seed=1, logit_gain=0.84)
    path = str(tmp_path / 'toy.npz')
    save_model(path, spec, params)
    return spec, params, path


@pytest.mark.parametrize('precision', ['f16', 'f32m', 'f64'])
def test_forward_coords01_matches_forward(cuda, tmp_path, precision):
    from metro_pose3d_amd import heads as MH, synth
    from metro_pose3d_amd.engine import Engine
    spec, params, _ = _toy_engine_model(tmp_path)
    eng = Engine(spec, params, precision, max_batch=130, device=cuda)
    images = torch.from_numpy(synth.make_images(130, spec.proc_side, seed=3)).to(cuda)
    for graphs in (0, 130):
        check(eng.lib.metro_plan_set_graph_max_batch(eng._plan, graphs), 'metro_plan_set_graph_max_batch')
        for n in (1, 64, 130):
            x = images[:n]
            base = eng.forward(x).clone()
            bufs = [torch.empty((n, spec.skeleton.n_head, 3), device=cuda) for _ in range(2)]
            ref = None
            for b, c01 in enumerate(bufs):
                for rep in range(3):                  # graphs on: first sight runs eagerly, then capture, then replay
                    for other in bufs:
                        other.fill_(-7.0)
                    poses = eng.forward(x, coords01=c01)
                    assert torch.equal(poses, base), (graphs, n, b, rep)
                    assert ((c01 >= 0) & (c01 <= 1)).all(), (graphs, n, b, rep)     # written: expectations in [0, 1]
                    ref = c01.clone() if ref is None else ref
                    assert torch.equal(c01, ref), (graphs, n, b, rep)
                    # the other buffer is a different graph key: nothing may land there
                    assert (bufs[1 - b] == -7.0).all(), (graphs, n, b, rep)
            assert torch.equal(eng.forward(x), base)
    n = 64
    x = images[:n]
    c01 = torch.full((n, spec.skeleton.n_head, 3), -7.0, device=cuda)
    poses = eng.forward(x, coords01=c01)
    assert ((c01 >= 0) & (c01 <= 1)).all()
    if precision == 'f64':
        li = [i for i, l in enumerate(eng.layer_infos()) if l.name.decode() == 'logits'][0]
        logits = eng.forward_upto(x, li)
        ref = MH.coords01_from_logits(logits, spec, precise=2)
        assert (c01 - ref).abs().max().item() <= 1e-6
    # heatmap_to_metric + root-relative + permutation of coords01 reproduces the poses: in fp32, the finalize's arithmetic, for
    # f16; in fp64 for f32m / f64, whose finalize decodes the fp64 expectation that coords01 holds rounded to fp32
    # (2200 mm x 6e-8 = 1.3e-4 mm per coordinate)
    dt = np.float32 if precision == 'f16' else np.float64
    c = c01.cpu().numpy().astype(dt)
    last = spec.proc_side - 1
    lrc, half = dt(last - last % spec.stride - 1), dt(spec.stride // 2)
    box, side = dt(spec.box_size_mm), dt(spec.proc_side)
    mm = np.concatenate([(c[..., :2] * lrc + half) * box / side, c[..., 2:] * box], -1)
    rel = (mm - mm[:, -1:])[:, list(spec.skeleton.permutation)]
    assert np.abs(rel - poses.cpu().numpy()).max() <= 1e-3, precision
    with pytest.raises(ValueError, match='coords01 must be'):
        eng.forward(x, coords01=torch.empty((n, 3, 3), device=cuda))
    eng.close()


@pytest.mark.parametrize('proc_side', [256, 384])
def test_locate_poses_in_frames_f64_matches_the_oracle(cuda, tmp_path, proc_side):
    """The model file's crop side reaches the crop, the forward and the placement: the oracle warps, runs and places at it."""
    from metro_pose3d_amd.frames import crop_params, estimate_pose_in_frames, locate_poses_in_frames, placement_params
    from oracle import forward as OF
    from tests import helpers as H
    from tests.test_gpu_frames import _cameras, _frame, _oracle_crops
    spec, params, path = _toy_engine_model(tmp_path, proc_side)
    d, cams = _cameras()
    cams[2].distortion_coeffs = None                                   # one undistorted camera: the homography keypoints
    frames = [_frame(*d[f'cam{i}_frame_hw'], seed=50 + i) for i in range(3)]
    sel = [0, 2, 8, 11, 14, 16, 19]
    boxes, fi = d['boxes'][sel], d['box_camera'][sel]
    n = len(sel)
    rng = np.random.default_rng(11)
    bones = rng.uniform(200, 450, len(spec.skeleton.head_edges))
    root = rng.uniform(3000, 5000, n)
    p = crop_params(cams, boxes, fi, proc_side)
    q = placement_params(cams, boxes, fi, proc_side)
    collect = {}
    OF.forward(H.oracle_spec(spec), params, _oracle_crops(frames, p, fi, proc_side), torch.float64, collect=collect)
    c01 = collect['coords01'].numpy().astype(np.float32)
    perm, mirror = spec.skeleton.permutation, spec.skeleton.out_mirror
    for scale, kw in (('bone-lengths', dict(bone_lengths=bones)), ('true-root-depth', dict(root_depth=root))):
        for coords in OPL.COORDS:
            got = locate_poses_in_frames(frames, boxes, path, cameras=cams, frame_index=fi, scale_recovery=scale,
                                         coords=coords, precision='f64', **kw)
            ref, kp, z = OPL.place(c01, q, spec.stride, scale, coords, perm, mirror, edges=spec.skeleton.head_edges,
                                   bone_lengths=bones, root_depth=root, proc_side=proc_side)
            assert got.poses.shape == (n, 17, 3) and got.keypoints2d.shape == (n, 17, 2) and got.z_offset.shape == (n,)
            assert np.abs(got.poses.cpu().numpy() - ref).max() <= 1e-2, (scale, coords)
            assert np.abs(got.keypoints2d.cpu().numpy() - kp).max() <= 1e-3, (scale, coords)
            assert np.abs(got.z_offset.cpu().numpy() - z).max() <= 1e-2
            assert got.joint_names[0] == b'pelv' and got.joint_edges.shape == (16, 2)
    for coords in OPL.COORDS:
        got = locate_poses_in_frames(frames, boxes, path, cameras=cams, frame_index=fi, scale_recovery='metro', coords=coords,
                                     precision='f64')
        base = estimate_pose_in_frames(frames, boxes, path, cameras=cams, frame_index=fi, coords=coords, precision='f64')[0]
        assert torch.equal(got.poses, base) and got.z_offset is None, coords
    # no cameras: keypoints through the square crops' homographies, 'metro' only
    got = locate_poses_in_frames(frames[0], boxes[:3], path, scale_recovery='metro', precision='f16')
    base = estimate_pose_in_frames(frames[0], boxes[:3], path, precision='f16')[0]
    assert torch.equal(got.poses, base) and torch.isfinite(got.keypoints2d).all()


# ---- the bone-length solve inside the placement launch, on the hard corpus ----------------------------------------------

def _random_rotations(rng, n, improper):
    """fp32 [n, 3, 3] orthogonal matrices; improper[i]: det -1 (a mirrored view)."""
    q, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    q *= (np.where(improper, -1.0, 1.0) * np.sign(np.linalg.det(q)))[:, None, None]
    return q.astype(np.float32)


def _synthetic_records(rng, inv_k):
    """PlacementParams around given K^-1: random rotations (every other one improper), camera positions metres away,
    identity keypoint homographies."""
    from metro_pose3d_amd.frames import PlacementParams
    n = len(inv_k)
    improper = np.arange(n) % 2 == 1
    eye = np.tile(np.eye(3, dtype=np.float32), (n, 1, 1))
    return PlacementParams(np.zeros(n, np.int32), np.asarray(inv_k, np.float32), _random_rotations(rng, n, improper),
                           _random_rotations(rng, n, improper), rng.uniform(-5000, 5000, (n, 3)).astype(np.float32), eye,
                           eye.copy(), np.zeros((n, 5), np.float32))


@pytest.mark.parametrize('family', ['friendly', 'noisy', 'mis-scaled', 'collapsed'])
@pytest.mark.parametrize('dataset', ['h36m', 'many19', 'merged'])
def test_place_poses_bone_lengths_on_the_hard_corpus(cuda, dataset, family):
    """metro_place_poses, bone-lengths, in the three coordinate frames on the corpus of tests/test_heads.py (130 crops, every
    other rotation improper, shared and per-pose targets): z_offset within the corpus tolerance of scipy's (tests/helpers.py
    BoneCase: max(1e-3 mm, k ulp32(|z|)), k from the oracle's own sensitivity to an ulp of its fp32 coefficients), no NaN
    where scipy is finite, poses against the oracle's placement of scipy's z, and every bit equal to
    metro_backproject_bone_lengths (+ metro_to_orig_cam + cam_loc) on the same inputs.
    Measured on the MI355X: z offsets and poses bit-equal to the oracle's in every family and frame."""
    from metro_pose3d_amd import heads as MH
    from tests import helpers as H
    for per_pose in (False, True):
        case = H.bone_case(dataset, family, per_pose)
        spec, sk = case.spec, case.spec.skeleton
        what = f'{dataset} {family} {"per-pose" if per_pose else "shared"}'
        q = _synthetic_records(np.random.default_rng(sk.n_head + per_pose), case.inv_k)
        crop, zhead = MH.backproject_bone_lengths(_dev(case.c01, cuda), case.inv_k, case.targets, spec, permute=True)
        for coords in OPL.COORDS:
            got, _, z = _place(cuda, spec, case.c01, q, 'bone-lengths', coords, bones=case.targets)
            assert np.array_equal(z, zhead.cpu().numpy()), (what, coords)
            same = crop
            if coords != 'crop':
                same = MH.to_orig_cam(crop, q.rot_to_orig_cam if coords == 'camera' else q.rot_to_world, sk.out_mirror)
            same = same.cpu().numpy() + (q.cam_loc[:, None] if coords == 'world' else np.float32(0))
            assert np.array_equal(got, same), (what, coords)
            case.check_z(z, f'{what} {coords}')
            ref, _, _ = OPL.place(case.c01, q, spec.stride, 'true-root-depth', coords, sk.permutation, sk.out_mirror,
                                  root_depth=case.z32, proc_side=spec.proc_side, centered=spec.centered_stride,
                                  box_size_mm=spec.box_size_mm)
            case.check_poses(got, ref, f'{what} {coords}')


# ---- placement outside the fixture: strides, centring, crop sides, skeletons, ragged n ----------------------------------

GRID = [('h36m', 4, True, 256), ('h36m', 8, False, 224), ('h36m', 16, True, 384), ('h36m', 32, False, 256),
        ('many19', 4, False, 384), ('many19', 8, True, 256), ('many19', 16, False, 224), ('many19', 32, True, 384),
        ('merged', 4, True, 224), ('merged', 8, False, 384), ('merged', 16, True, 256), ('merged', 32, False, 224)]


def _grid_case(dataset, stride, centered, side, n=200):
    """n synthetic crops of the fixture's three cameras (two distorted, one not: the keypoint modes alternate from crop to crop)
    with the virtual cameras of random person boxes; every other crop's rotations improper (a reflection that keeps rays in
    front of the camera), crops 4, 70 and 133 (distorted) and 8, 64 (homography) looking away from the camera.  coords01 are
    those of a pose 3 to 6 m in front of the virtual camera."""
    from metro_pose3d_amd.frames import placement_params
    from tests.test_frames import FIX as FRAMES_FIX, fixture_cameras
    fr = np.load(FRAMES_FIX)
    cams = fixture_cameras(fr)
    spec = ModelSpec(50, stride, dataset, centered_stride=centered, proc_side=side)
    sk = spec.skeleton
    rng = np.random.default_rng([stride, side, sk.n_head])
    fi = np.arange(n) % 3
    fi[64] = 2
    hw = np.array([fr[f'cam{i}_frame_hw'] for i in range(3)], np.float64)[fi]
    wh = rng.uniform(150, 500, (n, 2))
    xy = rng.uniform(0, 1, (n, 2)) * (hw[:, ::-1] - wh)
    q = placement_params(cams, np.concatenate([xy, wh], 1), fi, side)
    flip = np.diag([-1., 1., 1.]).astype(np.float32)
    back = np.diag([1., -1., -1.]).astype(np.float32)
    rc, rw, hm = q.rot_to_orig_cam.copy(), q.rot_to_world.copy(), q.homography.copy()
    rc[1::2] = rc[1::2] @ flip
    rw[1::2] = rw[1::2] @ flip
    for i in (4, 70, 133):
        assert q.keypoint_mode[i] == _lib.METRO_WARP_DISTORTED
        rc[i] = rc[i] @ back
    for i in (8, 64):
        assert q.keypoint_mode[i] == _lib.METRO_WARP_HOMOGRAPHY
        hm[i] = -hm[i]
    q = q._replace(rot_to_orig_cam=rc, rot_to_world=rw, homography=hm)
    assert (np.linalg.det(rc[1::2].astype(np.float64)) < 0).all() and (np.linalg.det(rc[0::2].astype(np.float64)) > 0).all()
    # a pose in front of each virtual camera and its soft-argmax coordinates
    j = sk.n_head
    p = rng.normal(0, 150, (n, j, 3))
    p[..., 2] += rng.uniform(3000, 6000, (n, 1))
    kk = np.linalg.inv(q.inv_intrinsics.astype(np.float64))
    uv = np.einsum('nij,ncj->nci', kk, p / p[..., 2:3])[..., :2]
    lrc = (side - 1) - ((side - 1) % stride) - 1
    c01 = np.empty((n, j, 3), np.float32)
    c01[..., :2] = (uv - (stride // 2 if centered else 0)) / lrc
    c01[..., 2] = (p[..., 2] - p[:, -1:, 2]) / spec.box_size_mm + 0.5 + rng.normal(0, 0.01, (n, j))
    edges = np.asarray(sk.head_edges)
    bones = np.linalg.norm(p[:, edges[:, 0]] - p[:, edges[:, 1]], axis=-1)
    rel = rng.normal(0, 300, (n, sk.n_out, 3)).astype(np.float32)
    return spec, q, c01, bones, p[:, -1, 2].astype(np.float32), rel


@pytest.mark.parametrize('dataset,stride,centered,side', GRID, ids=[f'{d}-s{s}-{"c" if c else "nc"}-{p}' for d, s, c, p in GRID])
def test_place_poses_outside_the_fixture(cuda, dataset, stride, centered, side):
    """metro_place_poses against tests/oracle_placement.py away from the reference fixture's one configuration: every stride
    with every skeleton, both centrings and crop sides 224 / 256 / 384 with every skeleton, n = 1, 64, 65 and 200, homography
    and distorted keypoints alternating inside a wave, every other rotation improper, five crops behind the camera (NaN
    keypoints exactly where the oracle has them).  All three scale recoveries in all three frames (bone-lengths: shared
    targets in one frame, per-pose targets in the two others).
    Bounds: those of test_place_poses_matches_the_reference, 1e-6 relative on 3D and on z, 1e-3 px on keypoints.
    Measured on the MI355X: 3D, z and keypoints bit-equal to the oracle's in all twelve configurations."""
    spec, q, c01, bones, root, rel = _grid_case(dataset, stride, centered, side)
    sk = spec.skeleton
    worst3 = worstkp = 0.0
    for k, n in enumerate((1, 64, 65, 200)):
        qn = type(q)(*(a[:n] for a in q))
        for s, scale in enumerate(OPL.SCALES):
            for c, coords in enumerate(OPL.COORDS):
                shared = (k + c) % 3 == 0
                t = (bones[:n].mean(axis=0) * 0.97 if shared else bones[:n]) if scale == 'bone-lengths' else None
                got, kp, z = _place(cuda, spec, c01[:n], qn, scale, coords, poses=rel[:n] if scale == 'metro' else None, bones=t,
                                    root=root[:n] if scale == 'true-root-depth' else None)
                want, wkp, wz = OPL.place(c01[:n], qn, stride, scale, coords, sk.permutation, sk.out_mirror, edges=sk.head_edges,
                                          bone_lengths=t, root_depth=root[:n], poses_rel=rel[:n], proc_side=side,
                                          centered=centered, box_size_mm=spec.box_size_mm)
                e3 = np.abs(got - want).max() / np.abs(want).max()
                assert e3 <= 1e-6, (n, scale, coords, e3)
                if scale != 'metro':
                    assert np.abs(z - wz).max() <= 1e-6 * np.abs(wz).max(), (n, scale, coords)
                assert np.array_equal(np.isnan(kp), np.isnan(wkp)), (n, scale, coords)
                behind = [i for i in (4, 8, 64, 70, 133) if i < n]
                assert np.isnan(wkp[behind]).all() and np.isnan(wkp).all(axis=(1, 2)).sum() == len(behind)
                ekp = np.nanmax(np.abs(kp - wkp)) if n > len(behind) else 0.0
                assert ekp <= 1e-3, (n, scale, coords, ekp)
                worst3, worstkp = max(worst3, e3), max(worstkp, ekp)
    print(f'{dataset} stride {stride} centred {centered} side {side}: worst 3D relative error {worst3:.2e}, worst keypoint '
          f'error {worstkp:.2e} px')
