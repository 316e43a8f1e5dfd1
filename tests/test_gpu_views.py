"""Test-time views on the MI355X (metro_expand_views, metro_merge_views, `views=` of estimate_pose_in_frames and
locate_poses_in_frames): one view reproduces the call without views bit for bit, copies of one view merge to its bits, the
device-expanded records against their host restatement (frames.view_params) and the crops cut through them, the whole call
against the oracle forward and the NumPy merge, and the mirror swap of a flipped view."""
import ctypes as C

import numpy as np
import pytest
import torch

from metro_pose3d_amd import _lib, frames as FR
from metro_pose3d_amd._lib import check
from metro_pose3d_amd.frames import (COORDS, SCALE_RECOVERY, estimate_pose_in_frames, locate_poses_in_frames, view_params,
                                     view_set)
from tests import oracle_placement as OPL, oracle_views as OV
from tests.test_gpu_frames import _cameras, _frame, _oracle_crops
from tests.test_gpu_placement import _toy_engine_model

pytestmark = pytest.mark.gpu

SEL = [0, 8, 11, 16, 19]          # boxes of the frames fixture: distorted cameras 0 and 1, the undistorted camera 2


def _scene(undistorted_last=True):
    d, cams = _cameras()
    if undistorted_last:
        cams[2].distortion_coeffs = None                  # the homography mode next to the distorted one
    frames = [_frame(*d[f'cam{i}_frame_hw'], seed=70 + i) for i in range(3)]
    return cams, frames, d['boxes'][SEL], d['box_camera'][SEL].astype(np.int64)


def _np(t):
    return None if t is None else t.cpu().numpy()


def _fields(raw, struct):
    """uint8 [m, sizeof] records -> {field: array [m, ...]}."""
    dt = np.dtype(struct)
    rec = np.ascontiguousarray(raw).view(dt).ravel()
    return {f: rec[f] for f in dt.names}


@pytest.mark.parametrize('precision', ['f16', 'f64'])
def test_one_view_is_bit_identical_to_no_views(cuda, tmp_path, precision):
    spec, _, path = _toy_engine_model(tmp_path)
    cams, frames, boxes, fi = _scene()
    bones = np.random.default_rng(2).uniform(200, 450, len(spec.skeleton.head_edges))
    for cameras in (cams, None):
        base = estimate_pose_in_frames(frames, boxes, path, cameras=cameras, frame_index=fi, precision=precision)[0]
        scale = dict(bone_lengths=bones) if cameras is not None else dict(scale_recovery='metro')
        ref = locate_poses_in_frames(frames, boxes, path, cameras=cameras, frame_index=fi, precision=precision, **scale)
        for views in (1, [(0, 1, False)], [(0.0, 1.0, np.bool_(False))]):
            got = estimate_pose_in_frames(frames, boxes, path, cameras=cameras, frame_index=fi, precision=precision, views=views)[0]
            assert torch.equal(got, base), (cameras is None, views)
            loc, spread = locate_poses_in_frames(frames, boxes, path, cameras=cameras, frame_index=fi, precision=precision,
                                                 views=views, return_spread=True, **scale)
            assert torch.equal(loc.poses, ref.poses) and (cameras is None or torch.equal(loc.z_offset, ref.z_offset))
            assert np.array_equal(_np(loc.keypoints2d), _np(ref.keypoints2d), equal_nan=True)
            assert (spread == 0).all() and spread.shape == (len(boxes), spec.skeleton.n_out)
        if cameras is None:
            crop = estimate_pose_in_frames(frames, boxes, path, frame_index=fi, precision=precision, coords='crop')[0]
            got = estimate_pose_in_frames(frames, boxes, path, frame_index=fi, precision=precision, coords='crop', views=1)[0]
            assert torch.equal(got, crop)


def test_no_views_is_the_identity_view_chain(cuda, tmp_path):
    """views=None is views=1 on host boxes and on device boxes, with and without cameras: no path skips the expansion or the
    merge.  f64: its forward gives a crop the same bits in any call."""
    spec, _, path = _toy_engine_model(tmp_path)
    cams, frames, boxes, fi = _scene()
    bones = np.random.default_rng(2).uniform(200, 450, len(spec.skeleton.head_edges))
    for cameras in (cams, None):
        scale = dict(bone_lengths=bones) if cameras is not None else dict(scale_recovery='metro')
        for geometry in ('host', 'device'):
            kw = dict(cameras=cameras, frame_index=fi, precision='f64', geometry=geometry)
            (none, s0), (one, s1) = (locate_poses_in_frames(frames, boxes, path, views=views, return_spread=True, **scale, **kw)
                                     for views in (None, 1))
            assert torch.equal(none.poses, one.poses), (cameras is None, geometry)
            if cameras is None:
                assert none.z_offset is None and one.z_offset is None
            else:
                assert torch.equal(none.z_offset, one.z_offset)
            assert np.array_equal(_np(none.keypoints2d), _np(one.keypoints2d), equal_nan=True)
            assert s0.shape == (len(boxes), spec.skeleton.n_out) and (s0 == 0).all() and torch.equal(s0, s1)
            rel = [estimate_pose_in_frames(frames, boxes, path, views=views, **kw)[0] for views in (None, 1)]
            assert torch.equal(rel[0], rel[1])


def test_improper_camera_rotation_is_one_answer(cuda, tmp_path):
    """A camera whose R has det -1: look_at_box builds a proper virtual R, so the identity view's rot_to_orig_cam has det -1
    and metro_merge_views takes keypoint j from joint mirror[j].  Host boxes with views=None, with views=1, and device boxes
    with views=None give one answer.  Before the chains were merged, host boxes with views=None never ran the merge: on these
    two boxes they returned the poses of the other two paths but the unswapped keypoints (row j of the others = their row
    mirror[j], up to 43.5 px apart), in 'metro' and 'bone-lengths' mode alike; views=1 and device boxes agreed bit for bit.
    The two boxes are camera 1's; the placement oracle puts every heat-map position of their crops in front of the camera, so
    the keypoints compared are finite."""
    spec, _, path = _toy_engine_model(tmp_path)
    sk = spec.skeleton
    cams, frames, boxes, fi = _scene()
    cams[1].R[0] *= -1
    boxes, fi = boxes[1:3], fi[1:3]
    assert (fi == 1).all() and np.linalg.det(cams[1].R.astype(np.float64)) < 0
    _, q = view_params(cams, boxes, fi, 1, 256)
    assert (np.linalg.det(q.rot_to_orig_cam.astype(np.float64)) < 0).all()
    c01 = np.random.default_rng(0).uniform(0, 1, (len(boxes), sk.n_head, 3)).astype(np.float32)
    assert np.isfinite(OPL.keypoints(c01, q, spec.stride, sk.permutation)).all()
    bones = np.random.default_rng(2).uniform(200, 450, len(sk.head_edges))
    for scale in (dict(scale_recovery='metro'), dict(scale_recovery='bone-lengths', bone_lengths=bones)):
        call = lambda **kw: locate_poses_in_frames(frames, boxes, path, cameras=cams, frame_index=fi, precision='f64',
                                                   **scale, **kw)
        host, one, device = call(), call(views=1), call(geometry='device')
        kp = _np(host.keypoints2d)
        assert np.isfinite(kp).all(axis=-1).mean() >= 0.5
        for other in (one, device):
            assert torch.equal(host.poses, other.poses), scale['scale_recovery']
            assert np.array_equal(kp, _np(other.keypoints2d), equal_nan=True), scale['scale_recovery']


def test_copies_of_one_view_merge_to_its_bits(cuda, tmp_path):
    """V copies of a rolled, zoomed, flipped view: the merge of V equal rows is that row (fp64 sums of <= 32 equal fp32 values
    are exact) and the spread is exactly 0.  f64: its forward gives a crop the same bits at any batch size."""
    spec, _, path = _toy_engine_model(tmp_path)
    cams, frames, boxes, fi = _scene()
    bones = np.random.default_rng(3).uniform(200, 450, len(spec.skeleton.head_edges))
    view = (12.5, 1.15, True)
    for cameras, scale in ((cams, dict(bone_lengths=bones)), (None, dict(scale_recovery='metro'))):
        one, s1 = locate_poses_in_frames(frames, boxes, path, cameras=cameras, frame_index=fi, precision='f64', views=[view],
                                         return_spread=True, **scale)
        many, s4 = locate_poses_in_frames(frames, boxes, path, cameras=cameras, frame_index=fi, precision='f64',
                                          views=[view] * 4, return_spread=True, **scale)
        assert torch.equal(one.poses, many.poses) and (s4 == 0).all() and (s1 == 0).all()
        assert np.array_equal(_np(one.keypoints2d), _np(many.keypoints2d), equal_nan=True)
        if cameras is not None:
            assert torch.equal(one.z_offset, many.z_offset)
        rel1 = estimate_pose_in_frames(frames, boxes, path, cameras=cameras, frame_index=fi, precision='f64', views=[view])[0]
        rel4 = estimate_pose_in_frames(frames, boxes, path, cameras=cameras, frame_index=fi, precision='f64', views=[view] * 4)[0]
        assert torch.equal(rel1, rel4)


def _ulps(a, b, scale, dt):
    return np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.spacing(np.asarray(scale, dt)).astype(np.float64)


def test_expanded_records_match_the_host_restatement(cuda):
    """metro_expand_views' records against frames.view_params: fp32 fields within 1 ulp, the fp64 partial homography within 4
    ulp.  A 3x3 entry's ulp is that of the largest entry of its column: a column multiplies one homogeneous coordinate, and
    entries that are 0 in exact arithmetic come out of LAPACK's solve as ~1e-20 where the closed-form inverse gives 0 (the
    homography's bottom row).  Crops cut through the device records are byte-identical to crops cut through the host records on
    every view whose records are bit-identical."""
    for undistorted in (True, False):
        cams, frames, boxes, fi = _scene(undistorted)
        views = [(0, 1, False), (-20, 1, False), (-7.5, 1.2, True), (20, 0.8, True), (3, 1, False), (0, 1.3, True)]
        vs = view_set(views)
        nv = len(views)
        for cameras in (cams, None):
            p, q = view_params(cameras, boxes, fi, views, 256)
            bases = FR.pack_view_bases(cameras, boxes, fi, 256)
            crops_raw, places_raw = FR._expand_views(bases, vs, 256, cuda)
            c, pl = _fields(_np(crops_raw), _lib.MetroCropWarp), _fields(_np(places_raw), _lib.MetroPlacement)
            m = len(boxes) * nv
            assert (c['frame'] == np.repeat(fi, nv)).all() and (c['mode'] == p.mode).all() and (pl['keypoint_mode'] == p.mode).all()
            f32 = [(c['homography'], p.homography), (pl['homography'], p.homography), (pl['inv_intrinsics'], q.inv_intrinsics),
                   (pl['rot_to_orig_cam'], q.rot_to_orig_cam), (pl['rot_to_world'], q.rot_to_world), (pl['cam_loc'], q.cam_loc),
                   (c['intrinsics'], p.intrinsics.reshape(m, 9)[:, :6]), (c['distortion'], p.distortion)]
            same = np.ones(m, bool)
            for got, want in f32:
                got, want = got.reshape(m, -1), np.asarray(want, np.float32).reshape(m, -1)
                scale = np.maximum(np.abs(got), np.abs(want))
                if got.shape[1] == 9:
                    scale = np.tile(scale.reshape(m, 3, 3).max(axis=1), (1, 3))
                u = _ulps(got, want, scale, np.float32)
                assert u.max() <= 1, u.max()
                same &= (got == want).all(axis=1)
            got, want = c['partial'].reshape(m, 3, 3), p.partial
            col = np.maximum(np.abs(got), np.abs(want)).max(axis=1, keepdims=True)
            assert _ulps(got, want, col, np.float64).max() <= 4
            same &= (got == want).all(axis=(1, 2))
            ident = np.tile([v == (0, 1, False) for v in views], len(boxes))
            assert same[ident].all()                                  # the identity view copies the box's records
            dev = torch.empty((m, 256, 256, 3), dtype=torch.float32, device=cuda)
            FR._launch_warp(FR._device_frames(frames, cuda), crops_raw, m, 256, dev, cuda)
            rows = np.flatnonzero(same)
            host = FR.warp_frames(frames, FR.CropParams(*(a[rows] for a in p)), np.repeat(fi, nv)[rows], 256, device=cuda)
            assert torch.equal(dev[rows], host)
            print(f'undistorted camera 2 {undistorted}, cameras {cameras is not None}: {len(rows)} of {m} views bit-identical '
                  f'records (byte-identical crops)')


def test_views_match_the_oracle_f64(cuda, tmp_path):
    """V = 5 (rolls, zooms other than 1, flips), distorted and undistorted cameras, every scale recovery: the merged call
    against the NumPy merge of per-view oracle placements, each view's crop cut by tests/oracle_frames.py from the host
    restatement's records and run through the oracle forward in fp64.  Poses within 1e-3 mm, keypoints within 1e-3 px."""
    from oracle import forward as OF
    from tests import helpers as H
    spec, params, path = _toy_engine_model(tmp_path)
    cams, frames, boxes, fi = _scene()
    views = [(-20, 1, False), (-8, 1.2, True), (0, 1, False), (9, 0.85, True), (20, 1.1, False)]
    nv, n = len(views), len(boxes)
    p, q = view_params(cams, boxes, fi, views, 256)
    fir = np.repeat(fi, nv)
    collect = {}
    rel = OF.forward(H.oracle_spec(spec), params, _oracle_crops(frames, p, fir, 256), torch.float64, collect=collect)
    c01 = collect['coords01'].numpy().astype(np.float32)
    rel = np.asarray(rel.numpy() if isinstance(rel, torch.Tensor) else rel, np.float32)
    perm, mirror = spec.skeleton.permutation, spec.skeleton.out_mirror
    rng = np.random.default_rng(5)
    bones = rng.uniform(200, 450, (n, len(spec.skeleton.head_edges)))
    root = rng.uniform(3000, 5000, n)
    worst3, worstkp = 0.0, 0.0
    for scale, kw in (('metro', {}), ('bone-lengths', dict(bone_lengths=bones)), ('true-root-depth', dict(root_depth=root))):
        for coords in ('camera', 'world'):
            got, spread = locate_poses_in_frames(frames, boxes, path, cameras=cams, frame_index=fi, scale_recovery=scale,
                                                 coords=coords, precision='f64', views=views, return_spread=True, **kw)
            pv, kv, zv = OPL.place(c01, q, spec.stride, scale, coords, perm, mirror, edges=spec.skeleton.head_edges,
                                   bone_lengths=np.repeat(bones, nv, axis=0), root_depth=np.repeat(root, nv), poses_rel=rel)
            rot = q.rot_to_orig_cam
            want, wkp, wz, wsp = OV.merge(pv, kv, zv, rot, mirror, nv)
            e3 = np.abs(_np(got.poses) - want).max()
            ekp = np.nanmax(np.abs(_np(got.keypoints2d) - wkp))
            assert np.array_equal(np.isnan(_np(got.keypoints2d)), np.isnan(wkp))
            worst3, worstkp = max(worst3, e3), max(worstkp, ekp)
            assert e3 <= 1e-3, (scale, coords, e3)
            assert ekp <= 1e-3, (scale, coords, ekp)
            assert np.abs(_np(spread) - wsp).max() <= 1e-3
            if scale != 'metro':
                assert np.abs(_np(got.z_offset) - wz).max() <= 1e-3
            else:
                assert got.z_offset is None
    print(f'views vs oracle: worst 3D {worst3:.2e} mm, worst keypoint {worstkp:.2e} px')


def test_flipped_view_swaps_mirror_joints(cuda, tmp_path):
    """A flipped view in metro mode against the single-view machinery on the same crop (its device records, the engine's
    forward, one metro_place_poses launch): the merge carries the 3D poses as placed (joint j = R . crop pose of mirror[j])
    and takes keypoint j from the mirror joint's frame pixel."""
    from metro_pose3d_amd.inference import _engine_for
    spec, _, path = _toy_engine_model(tmp_path)
    cams, frames, boxes, fi = _scene()
    sk = spec.skeleton
    mirror = np.asarray(sk.out_mirror)
    assert (mirror != np.arange(sk.n_out)).any()
    vs = view_set([(0, 1, True)])
    got = locate_poses_in_frames(frames, boxes, path, cameras=cams, frame_index=fi, scale_recovery='metro', precision='f32m',
                                 views=[(0, 1, True)])
    n = len(boxes)
    with torch.cuda.device(cuda):
        eng = _engine_for(path, 'f32m', cuda, n)
        crops, places = FR._warp_views(frames, cams, boxes, fi, vs, 256, cuda)
        rel = torch.empty((n, sk.n_out, 3), device=cuda)
        c01 = torch.empty((n, sk.n_head, 3), device=cuda)
        eng.forward(crops, out=rel, coords01=c01)
        out = torch.empty((n, sk.n_out, 3), device=cuda)
        kp = torch.empty((n, sk.n_out, 2), device=cuda)
        d_mirror = torch.from_numpy(mirror.astype(np.int32)).to(cuda)
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
        check(_lib.load().metro_place_poses(ptr(c01), ptr(rel), ptr(places), n, C.byref(eng.cspec), SCALE_RECOVERY['metro'],
                                            None, 0, None, None, 0, ptr(d_mirror), COORDS['camera'], ptr(out), ptr(kp), None,
                                            C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)), 'metro_place_poses')
    rot = _fields(_np(places), _lib.MetroPlacement)['rot_to_orig_cam'].reshape(n, 3, 3)
    assert (np.linalg.det(rot.astype(np.float64)) < 0).all()
    assert torch.equal(got.poses, out)
    expect = np.einsum('nij,nkj->nki', rot.astype(np.float64), _np(rel).astype(np.float64)[:, mirror])
    assert np.abs(_np(out) - expect).max() <= 1e-3
    assert np.array_equal(_np(got.keypoints2d), _np(kp)[:, mirror], equal_nan=True)
    assert not np.allclose(_np(kp)[:, mirror], _np(kp), equal_nan=True)       # the swap moves the keypoints


# ---- metro_merge_views on its own against fp64 ----------------------------------------------------------------------------

def _merge_reference(poses, kps, z, rot, mirror, nv):
    """Plain fp64: per box and joint the mean over the views, the RMS distance of the views from it, the mean of the finite
    keypoints (a view with det <= 0 contributes its mirror joint's), the mean z offset."""
    p = poses.astype(np.float64).reshape(-1, nv, *poses.shape[1:])
    mean = p.sum(axis=1) / nv
    spread = np.sqrt(((p - mean[:, None]) ** 2).sum(axis=-1).sum(axis=1) / nv)
    k = kps.astype(np.float64).reshape(-1, nv, *kps.shape[1:])
    mirrored = ~(np.linalg.det(rot.astype(np.float64)) > 0).reshape(-1, nv)
    k = np.where(mirrored[:, :, None, None], k[:, :, list(mirror)], k)
    ok = np.isfinite(k).all(axis=-1, keepdims=True)
    cnt = ok.sum(axis=1)
    with np.errstate(invalid='ignore', divide='ignore'):
        kp = np.where(cnt > 0, np.where(ok, k, 0.0).sum(axis=1) / cnt, np.nan)
    return mean, spread, kp, z.astype(np.float64).reshape(-1, nv).sum(axis=1) / nv


def _within_one_ulp(got, want64):
    """got fp32 against the fp64 result rounded to fp32: equal, or one float32 spacing apart."""
    want = want64.astype(np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ok = ~np.isnan(want)
    return (d[ok] <= np.spacing(np.abs(want[ok])).astype(np.float64)).all(), int((got[ok] != want[ok]).sum())


@pytest.mark.parametrize('nj', [17, 19, 53])
@pytest.mark.parametrize('nv', [1, 2, 5, 32])
def test_merge_views_matches_fp64(cuda, lib, nv, nj):
    """metro_merge_views called directly, V = 1 / 2 / 5 / 32 views of 17 / 19 / 53 joints, n such that n x joints crosses one
    and two 256-thread blocks.  Views 1, 4, 7, ... are mirrored (det -1: keypoint j comes from joint mirror[j]), one record has
    det exactly 0 (counts as mirrored, as metro_place_poses decides it).  Planted among the keypoints: NaN or +-inf in ONE
    coordinate (the view drops out of both), every view of a joint and of its mirror joint non-finite (NaN out), and boxes
    with none.  The kernel accumulates in fp64 in view order, so poses, spread, keypoints and z are expected bit-equal to the
    fp64 reference rounded to fp32; asserted: within one float32 ulp of it, and the NaN pattern identical.  Outputs that
    are not asked for (no spread; no keypoints and z) change nothing else, and a guard row behind every output stays as it
    was.  Measured on the MI355X: every value bit-equal."""
    from metro_pose3d_amd.frames import PlacementParams, pack_placements
    from metro_pose3d_amd.joints import skeleton
    from tests.test_gpu_placement import _random_rotations
    sk = skeleton({17: 'h36m', 19: 'many19', 53: 'merged'}[nj])
    mirror = np.asarray(sk.head_mirror if nj == 53 else sk.out_mirror, np.int32)
    assert len(mirror) == nj and (mirror != np.arange(nj)).any()
    differ = 0
    for n in (256 // nj + 1, 512 // nj + 1):
        assert (n - 1) * nj <= 256 * ((n * nj - 1) // 256) < n * nj            # the last box spills into one more block
        rng = np.random.default_rng([nv, nj, n])
        m = n * nv
        poses = (rng.normal(0, 400, (m, nj, 3)) + rng.uniform(-5000, 5000, (m, 1, 3))).astype(np.float32)
        kps = rng.uniform(-200, 2200, (m, nj, 2)).astype(np.float32)
        z = rng.uniform(2000, 7000, m).astype(np.float32)
        rot = _random_rotations(rng, m, np.arange(m) % 3 == 1)
        rot[m // 2] = np.diag([1., 1., 0.]).astype(np.float32)                  # det exactly 0
        bad = np.array([np.nan, np.inf, -np.inf], np.float32)
        for i in range(0, m, 3):                                               # one coordinate of one joint of a view
            kps[i, rng.integers(nj), rng.integers(2)] = bad[i % 3]
        for box in range(0, n, 4):                                             # every view of a joint and of its mirror joint
            j = int(rng.integers(nj))
            kps[box * nv:(box + 1) * nv, [j, mirror[j]], rng.integers(2)] = bad[box % 3]
        eye = np.tile(np.eye(3, dtype=np.float32), (m, 1, 1))
        recs = pack_placements(PlacementParams(np.zeros(m, np.int32), eye, rot, eye, np.zeros((m, 3), np.float32), eye, eye,
                                               np.zeros((m, 5), np.float32)))
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
        d_p, d_k, d_z, d_r, d_m = dev(poses), dev(kps), dev(z), dev(recs), dev(mirror)
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)

        def run(with_kp, with_z, with_spread):
            """-> host arrays (None where not asked for), each allocated with a guard row that must stay 12345."""
            outs = [torch.full(s, 12345.0, device=cuda) for s in ((n + 1, nj, 3), (n + 1, nj, 2), (n + 1,), (n + 1, nj))]
            use = [True, with_kp, with_z, with_spread]
            o = [t if u else None for t, u in zip(outs, use)]
            check(lib.metro_merge_views(ptr(d_p), ptr(d_k if with_kp else None), ptr(d_z if with_z else None), ptr(d_r), ptr(d_m),
                                        n, nv, nj, ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]),
                                        C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)), 'metro_merge_views')
            for t in outs:
                assert (t[n:] == 12345.0).all()
            return [t[:n].cpu().numpy() if u else None for t, u in zip(outs, use)]

        want = _merge_reference(poses, kps, z, rot, mirror, nv)
        got = run(True, True, True)
        assert np.isnan(want[2]).any() and np.isfinite(want[2]).any()
        for name, g, w in zip(('poses', 'keypoints', 'z', 'spread'), (got[0], got[1], got[2], got[3]),
                              (want[0], want[2], want[3], want[1])):
            ok, ne = _within_one_ulp(g, w)
            differ += ne
            assert ok, (n, name)
        if nv == 1:
            assert (got[3] == 0).all() and np.array_equal(got[0], poses)
        bare = run(False, False, False)
        assert np.array_equal(bare[0], got[0]) and bare[1] is None
        some = run(True, False, False)
        assert np.array_equal(some[0], got[0]) and np.array_equal(some[1], got[1], equal_nan=True)
    print(f'V {nv}, {nj} joints: {differ} values differ from the rounded fp64 reference')
