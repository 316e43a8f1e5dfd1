"""Crop geometry on the MI355X (metro_look_at_boxes, frames.look_at_boxes, `geometry=` of estimate_pose_in_frames and
locate_poses_in_frames): the device's MetroViewBase records against the host's (pack_view_bases) and against the reference's
own camera values, the crops cut through them, whole calls with CUDA boxes against host boxes, and the frame-index status."""
import numpy as np
import pytest
import torch

from metro_pose3d_amd import frames as FR
from metro_pose3d_amd.frames import estimate_pose_in_frames, locate_poses_in_frames, look_at_boxes, pack_view_bases, view_set
from tests.test_frames import FIX, fixture_cameras
from tests.test_gpu_placement import _toy_engine_model
from tests.test_gpu_views import _np, _scene, _ulps

pytestmark = pytest.mark.gpu

# boxes inside the frame, partly outside, wholly outside, tall and wide (frames of the fixture cameras: 1000 x 1000,
# 2048 x 2048 and 720 x 1280)
EXTRA_BOXES = np.array([[-4000, 200, 300, 400], [1300, 1300, 150, 200], [-900, -900, 300, 300], [100, 100, 50, 400],
                        [100, 100, 600, 80], [500, 300, 200, 200], [-60, 500, 240, 230]])
EXTRA_CAMERA = np.array([2, 0, 1, 0, 1, 2, 1])
# Measured on the MI355X: 1 ulp and 2.2e-16 (the closed-form inverses against LAPACK's), and 17 to 27 of the 27 records per
# camera set bit-identical.  The bounds keep one ulp for a host whose BLAS adds its fp32 products in another order.
F32_ULPS = 2              # fp32 fields, column-scaled ulp
F64_REL = 1e-15           # fp64 fields that derive from fp32 values, column-scaled relative


def _records(raw):
    return np.frombuffer(np.ascontiguousarray(raw).tobytes(), FR.VIEW_BASE_DTYPE)


def _camera_sets():
    """(name, cameras): the fixture's H36M-like and 3DHP distorted cameras with the intrinsics-only one undistorted, with
    zero coefficients, every camera undistorted; one Camera for all frames; None."""
    d = np.load(FIX)
    out = []
    for variant in ('fixture', 'zero coefficients', 'undistorted'):
        cams = fixture_cameras(d)
        if variant == 'zero coefficients':
            cams[2].distortion_coeffs = np.zeros(5, np.float32)
        if variant == 'undistorted':
            for c in cams:
                c.distortion_coeffs = None
        out += [(variant, cams), (variant + ', one camera', cams[1])]
    return out + [('no camera', None)]


def _boxes():
    d = np.load(FIX)
    return np.concatenate([d['boxes'], EXTRA_BOXES]), np.concatenate([d['box_camera'], EXTRA_CAMERA]).astype(np.int64)


def _compare(got, want):
    """-> (rows bit-identical, worst fp32 ulp, worst fp64 relative); asserts the bounds."""
    n = len(want)
    same = np.ones(n, bool)
    worst32, worst64 = 0.0, 0.0
    for f in FR.VIEW_BASE_DTYPE.names:
        g, w = got[f].reshape(n, -1), want[f].reshape(n, -1)
        if g.dtype.kind == 'i':
            assert (g == w).all(), f
            continue
        assert np.array_equal(np.isnan(g), np.isnan(w)), f               # degenerate boxes: the host's NaN records
        same &= ((g == w) | np.isnan(g)).all(axis=1)
        g, w = np.nan_to_num(g), np.nan_to_num(w)
        scale = np.maximum(np.abs(g), np.abs(w))
        if g.shape[1] == 9:
            scale = np.tile(scale.reshape(n, 3, 3).max(axis=1), (1, 3))
        if g.dtype == np.float32 or f == 'virt_r':           # virt_r: the fp32 R stored as fp64
            u = _ulps(g, w, scale, np.float32).max()
            assert u <= F32_ULPS, (f, u)
            worst32 = max(worst32, u)
        elif f == 'orig_r':
            assert (g == w).all()
        else:
            r = (np.abs(g - w) / np.where(scale > 0, scale, 1)).max()
            assert r <= F64_REL, (f, r)
            worst64 = max(worst64, r)
    return same, worst32, worst64


def test_device_bases_match_pack_view_bases(cuda):
    """metro_look_at_boxes' records against pack_view_bases' on the same boxes: integer fields equal, fp32 fields within
    F32_ULPS column-scaled ulp, the fp64 fields that derive from fp32 values (virt_k, partial, old_matrix) within F64_REL
    column-scaled; cameras=None bit-identical (box_homography: a few fp64 operations and a cast)."""
    boxes, fi = _boxes()
    for name, cameras in _camera_sets():
        want = _records(pack_view_bases(cameras, boxes, fi, 256))
        for db, dfi in ((torch.from_numpy(boxes).to(cuda), torch.from_numpy(fi).to(cuda)), (boxes, fi)):
            got = _records(_np(look_at_boxes(cameras, db, dfi, 256, n_frames=3)))
            same, u32, r64 = _compare(got, want)
            if cameras is None:
                assert same.all()
        print(f'{name}: {same.sum()} of {len(boxes)} records bit-identical; worst fp32 field {u32:.0f} ulp, worst fp64 field '
              f'{r64:.1e} relative')


def test_device_cameras_match_the_reference(cuda):
    """The device's virtual cameras and rotations back against the reference's own values (tests/golden/ref_frames_v1.npz),
    at the tolerances the host path meets in tests/test_frames.py."""
    d = np.load(FIX)
    cams = fixture_cameras(d)
    got = _records(_np(look_at_boxes(cams, torch.from_numpy(d['boxes']).to(cuda), d['box_camera'], int(d['side']))))
    n = len(got)
    assert np.allclose(got['virt_k'].reshape(n, 3, 3), d['virt_k'], rtol=1e-6, atol=0)
    assert np.allclose(got['virt_r'].reshape(n, 3, 3), d['virt_r'], rtol=1e-6, atol=1e-7)
    assert np.allclose(got['rot_to_orig_cam'].reshape(n, 3, 3), d['rot_to_orig_cam'], atol=1e-6)
    assert np.allclose(got['rot_to_world'].reshape(n, 3, 3), d['rot_to_world'], atol=1e-6)


def test_crops_through_device_records(cuda):
    """Crops cut through the device records (identity view, one warp launch) are byte-identical to crops cut through the host
    records on every row whose records are bit-identical, and at least 99.9 % of all crop values are identical."""
    vs = view_set(1)
    for undistorted in (True, False):
        cams, frames, boxes, fi = _scene(undistorted)
        boxes = np.concatenate([boxes, EXTRA_BOXES[:4]])
        fi = np.concatenate([fi, EXTRA_CAMERA[:4]]).astype(np.int64)
        n = len(boxes)
        for cameras in (cams, None):
            host = pack_view_bases(cameras, boxes, fi, 256)
            dev = look_at_boxes(cameras, torch.from_numpy(boxes).to(cuda), torch.from_numpy(fi).to(cuda), 256, n_frames=3)
            same = (_np(dev) == host).all(axis=1)
            out = []
            for bases in (host, dev):
                recs, _ = FR._expand_views(bases, vs, 256, cuda)
                crops = torch.empty((n, 256, 256, 3), dtype=torch.float32, device=cuda)
                FR._launch_warp(FR._device_frames(frames, cuda), recs, n, 256, crops, cuda)
                out.append(crops)
            rows = torch.from_numpy(np.flatnonzero(same)).to(cuda)
            assert torch.equal(out[0][rows], out[1][rows])
            frac = (out[0] == out[1]).double().mean().item()
            assert frac >= 0.999, frac
            print(f'undistorted camera 2 {undistorted}, cameras {cameras is not None}: {same.sum()} of {n} records '
                  f'bit-identical, {100 * frac:.4f} % of crop values identical')


def test_calls_with_cuda_boxes_match_host_boxes(cuda, tmp_path):
    """estimate_pose_in_frames and locate_poses_in_frames (bone-lengths, distorted and undistorted cameras, camera and world
    coords, views=None and 5, return_spread) with CUDA boxes against host boxes of the same values, f64: poses within 0.1 mm,
    keypoints within 1e-2 px, z offsets within 0.1 mm.  geometry='device' with host boxes gives the bits of CUDA boxes.
    Measured on the MI355X: every maximum 0 (poses, keypoints and z offsets bit-identical: the records differ by at most one
    fp32 ulp, and no crop value moved)."""
    spec, _, path = _toy_engine_model(tmp_path)
    bones = np.random.default_rng(7).uniform(200, 450, len(spec.skeleton.head_edges))
    worst = np.zeros(3)
    for undistorted in (True, False):
        cams, frames, boxes, fi = _scene(undistorted)
        dboxes, dfi = torch.from_numpy(boxes).to(cuda), torch.from_numpy(fi).to(cuda)
        for views in (None, 5):
            for coords in ('camera', 'world'):
                kw = dict(cameras=cams, precision='f64', views=views, coords=coords)
                want = estimate_pose_in_frames(frames, boxes, path, frame_index=fi, **kw)[0]
                got = estimate_pose_in_frames(frames, dboxes, path, frame_index=dfi, **kw)[0]
                same = estimate_pose_in_frames(frames, boxes, path, frame_index=fi, geometry='device', **kw)[0]
                assert torch.equal(got, same)
                e = (got - want).abs().max().item()
                assert e <= 0.1, (undistorted, views, coords, e)
                worst[0] = max(worst[0], e)
                lw, sw = locate_poses_in_frames(frames, boxes, path, frame_index=fi, bone_lengths=bones, return_spread=True, **kw)
                lg, sg = locate_poses_in_frames(frames, dboxes, path, frame_index=dfi, bone_lengths=bones, return_spread=True,
                                                **kw)
                ls = locate_poses_in_frames(frames, boxes, path, frame_index=fi, bone_lengths=bones, geometry='device', **kw)
                assert torch.equal(lg.poses, ls.poses) and torch.equal(lg.z_offset, ls.z_offset)
                assert np.array_equal(_np(lg.keypoints2d), _np(ls.keypoints2d), equal_nan=True)
                e3 = (lg.poses - lw.poses).abs().max().item()
                ekp = np.nanmax(np.abs(_np(lg.keypoints2d) - _np(lw.keypoints2d)))
                assert np.array_equal(np.isnan(_np(lg.keypoints2d)), np.isnan(_np(lw.keypoints2d)))
                ez = (lg.z_offset - lw.z_offset).abs().max().item()
                assert e3 <= 0.1 and ekp <= 1e-2 and ez <= 0.1, (undistorted, views, coords, e3, ekp, ez)
                assert (sg - sw).abs().max().item() <= 0.1
                worst = np.maximum(worst, [e, max(e3, ez), ekp])
    print(f'CUDA boxes vs host boxes, f64: worst root-relative pose {worst[0]:.2e} mm, worst absolute pose / z offset '
          f'{worst[1]:.2e} mm, worst keypoint {worst[2]:.2e} px')


def test_box_dtypes_frame_indices_and_empty_calls(cuda, tmp_path):
    """float32 and float64 CUDA boxes of exactly representable values give the same poses, a device frame_index the poses of
    the host one, and n = 0 returns empty results."""
    spec, _, path = _toy_engine_model(tmp_path)
    cams, frames, boxes, fi = _scene(False)
    boxes = np.round(boxes * 4) / 4                                   # quarter pixels: exact in fp32
    bones = np.random.default_rng(8).uniform(200, 450, len(spec.skeleton.head_edges))
    b64, b32 = torch.from_numpy(boxes).to(cuda), torch.from_numpy(boxes.astype(np.float32)).to(cuda)
    for views in (None, 3):
        a = estimate_pose_in_frames(frames, b64, path, cameras=cams, frame_index=fi, precision='f64', views=views)[0]
        b = estimate_pose_in_frames(frames, b32, path, cameras=cams, frame_index=torch.from_numpy(fi).to(cuda),
                                    precision='f64', views=views)[0]
        c = estimate_pose_in_frames(frames, b32, path, cameras=cams, frame_index=torch.from_numpy(fi.astype(np.int32)).to(cuda),
                                    precision='f64', views=views)[0]
        assert torch.equal(a, b) and torch.equal(a, c)
        la = locate_poses_in_frames(frames, b64, path, cameras=cams, frame_index=fi, bone_lengths=bones, precision='f64',
                                    views=views)
        lb = locate_poses_in_frames(frames, b32, path, cameras=cams, frame_index=torch.from_numpy(fi).to(cuda),
                                    bone_lengths=bones, precision='f64', views=views)
        assert torch.equal(la.poses, lb.poses) and torch.equal(la.z_offset, lb.z_offset)
    empty = torch.zeros((0, 4), dtype=torch.float32, device=cuda)
    e = estimate_pose_in_frames(frames, empty, path, cameras=cams, frame_index=torch.zeros(0, dtype=torch.int64, device=cuda),
                                precision='f64')[0]
    assert e.shape == (0, spec.skeleton.n_out, 3)
    le = locate_poses_in_frames(frames, empty, path, cameras=cams, bone_lengths=bones, precision='f64', views=5)
    assert le.poses.shape == (0, spec.skeleton.n_out, 3) and le.keypoints2d.shape == (0, spec.skeleton.n_out, 2)
    assert look_at_boxes(cams, empty, None, 256).shape == (0, FR.VIEW_BASE_DTYPE.itemsize)


def test_device_boxes_take_no_host_geometry(cuda, tmp_path, monkeypatch):
    """With CUDA boxes nothing on the per-box path calls the host geometry."""
    spec, _, path = _toy_engine_model(tmp_path)
    cams, frames, boxes, fi = _scene(False)
    bones = np.random.default_rng(9).uniform(200, 450, len(spec.skeleton.head_edges))
    dboxes, dfi = torch.from_numpy(boxes).to(cuda), torch.from_numpy(fi).to(cuda)
    want = estimate_pose_in_frames(frames, dboxes, path, cameras=cams, frame_index=dfi, precision='f64')[0]
    lwant = locate_poses_in_frames(frames, dboxes, path, cameras=cams, frame_index=dfi, bone_lengths=bones, precision='f64',
                                   views=5)

    def boom(*a, **k):
        raise AssertionError('per-box host geometry on the device path')

    for name in ('look_at_box', 'crop_params', 'placement_params', 'pack_crops', 'pack_placements', 'pack_view_bases',
                 '_frame_params_and_cameras'):
        monkeypatch.setattr(FR, name, boom)
    for cameras in (cams, None):
        estimate_pose_in_frames(frames, dboxes, path, cameras=cameras, frame_index=dfi, precision='f64', views=3)
    got = estimate_pose_in_frames(frames, dboxes, path, cameras=cams, frame_index=dfi, precision='f64')[0]
    lgot = locate_poses_in_frames(frames, dboxes, path, cameras=cams, frame_index=dfi, bone_lengths=bones, precision='f64',
                                  views=5)
    assert torch.equal(got, want) and torch.equal(lgot.poses, lwant.poses)


def test_device_frame_index_out_of_range_raises(cuda, tmp_path):
    """A device frame index outside [0, n_frames) is clamped by the kernel (no read outside the tables) and reported: the call
    raises ValueError; a valid call right after it in the same process returns the expected poses."""
    spec, _, path = _toy_engine_model(tmp_path)
    cams, frames, boxes, fi = _scene(False)
    bones = np.random.default_rng(10).uniform(200, 450, len(spec.skeleton.head_edges))
    dboxes = torch.from_numpy(boxes).to(cuda)
    want = estimate_pose_in_frames(frames, dboxes, path, cameras=cams, frame_index=torch.from_numpy(fi).to(cuda),
                                   precision='f64')[0]
    lwant = locate_poses_in_frames(frames, dboxes, path, cameras=cams, frame_index=torch.from_numpy(fi).to(cuda),
                                   bone_lengths=bones, precision='f64')
    for bad_value in (-1, 3, 1 << 40):
        bad = torch.from_numpy(fi).to(cuda)
        bad[1] = bad_value
        with pytest.raises(ValueError, match='frame_index'):
            estimate_pose_in_frames(frames, dboxes, path, cameras=cams, frame_index=bad, precision='f64')
        for check_finite in (True, False):
            with pytest.raises(ValueError, match='frame_index'):
                locate_poses_in_frames(frames, dboxes, path, cameras=cams, frame_index=bad, bone_lengths=bones, precision='f64',
                                       views=2, check_finite=check_finite)
        with pytest.raises(ValueError, match='frame_index'):
            look_at_boxes(cams, dboxes, bad, 256, n_frames=3)
    with pytest.raises(ValueError, match='frame_index'):                 # host indices: checked before any launch
        estimate_pose_in_frames(frames, dboxes, path, cameras=cams, frame_index=np.where(fi == 2, 5, fi), precision='f64')
    got = estimate_pose_in_frames(frames, dboxes, path, cameras=cams, frame_index=torch.from_numpy(fi).to(cuda),
                                  precision='f64')[0]
    lgot = locate_poses_in_frames(frames, dboxes, path, cameras=cams, frame_index=torch.from_numpy(fi).to(cuda),
                                  bone_lengths=bones, precision='f64')
    assert torch.equal(got, want) and torch.equal(lgot.poses, lwant.poses)

