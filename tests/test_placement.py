"""Absolute poses and frame keypoints (frames.placement_params, frames.locate_poses_in_frames, metro_place_poses): the host
geometry and the NumPy oracle of the placement chain against the reference's own code (tests/golden/ref_placement_v1.npz,
made by tests/golden/make_ref_placement.py), a known-answer round trip, the MetroPlacement layout and the API's argument
checks.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from metro_pose3d_amd import ModelSpec, _lib, save_model, synth
from metro_pose3d_amd.frames import Camera, crop_params, locate_poses_in_frames, look_at_box, pack_placements, placement_params
from metro_pose3d_amd.joints import skeleton
from tests import oracle_placement as OPL
from tests.test_frames import fixture_cameras

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, 'tests', 'golden', 'ref_placement_v1.npz')
FRAMES_FIX = os.path.join(ROOT, 'tests', 'golden', 'ref_frames_v1.npz')
SK = skeleton('h36m')


def fixture_params():
    d, fr = np.load(FIX), np.load(FRAMES_FIX)
    return d, placement_params(fixture_cameras(fr), d['boxes'], d['box_camera'], int(d['side']))


def test_placement_params_match_the_reference():
    d, q = fixture_params()
    fr = np.load(FRAMES_FIX)
    assert q.inv_intrinsics.dtype == np.float32 and q.cam_loc.dtype == np.float32
    # look_at_box agrees with the reference's to rtol 1e-6 (tests/test_frames.py); its inverse in fp32 within a few ulp
    assert np.allclose(q.inv_intrinsics, d['inv_k'], rtol=2e-6, atol=1e-9)
    assert np.allclose(q.rot_to_orig_cam, d['rot_to_orig_cam'], atol=1e-6)
    assert np.allclose(q.rot_to_world, d['rot_to_world'], atol=1e-6)
    assert np.array_equal(q.cam_loc, d['cam_loc'])
    distorted = d['box_camera'] < 2
    assert (q.keypoint_mode == np.where(distorted, _lib.METRO_WARP_DISTORTED, _lib.METRO_WARP_HOMOGRAPHY)).all()
    # the keypoint homography of an undistorted camera IS the warp's crop -> frame matrix; it maps crop pixels to the pixels
    # the reference's general branch gives
    p = crop_params(fixture_cameras(fr), d['boxes'], d['box_camera'], int(d['side']))
    assert np.array_equal(q.homography, p.homography)
    cams = fixture_cameras(fr)
    for i in np.flatnonzero(~distorted):
        virt = look_at_box(cams[d['box_camera'][i]], d['boxes'][i], int(d['side']))
        uv = np.array([[10., 20.], [128., 128.], [250., 3.]])
        h = np.concatenate([uv, np.ones((3, 1))], 1) @ q.homography[i].astype(np.float64).T
        orig = cams[d['box_camera'][i]]
        world = virt.camera_to_world(virt.image_to_camera(uv))
        want = orig.camera_to_image_undistorted(orig.world_to_camera(world))
        assert np.allclose(h[:, :2] / h[:, 2:], want, atol=1e-3), i


def test_no_camera_keeps_the_square_crop():
    q = placement_params(None, [[10, 20, 100, 200]], [0], 256)
    assert (q.inv_intrinsics == 0).all() and (q.rot_to_orig_cam == np.eye(3)).all() and (q.cam_loc == 0).all()
    assert q.keypoint_mode[0] == _lib.METRO_WARP_HOMOGRAPHY
    h = q.homography[0].astype(np.float64)
    for crop_px, frame_px in (((-0.5, -0.5), (-40.0, 20.0)), ((255.5, 255.5), (160.0, 220.0))):   # crop corners -> square's corners
        p = h @ [crop_px[0], crop_px[1], 1]
        assert np.allclose(p[:2] / p[2] + 0.5, frame_px, atol=1e-4)


@pytest.mark.parametrize('scale', OPL.SCALES)
def test_placement_oracle_matches_the_reference(scale):
    """The placement chain (what metro_place_poses computes) on the fixture's inputs against the reference's outputs.
    3D: 1e-6 relative (the same fp32 formulas up to the einsum's summation order and our look_at_box's last-bit differences;
    measured: bit-equal); keypoints: 1e-3 px (fp32 rays through the fp32 K^-1 and rotation instead of the reference's
    undistortPoints in fp64 and its world round trip: ~1e-7 relative of a 1000-2000 px focal length; measured 2.4e-4 px)."""
    d, q = fixture_params()
    perm = list(range(SK.n_head))                    # the fixture is in head order
    mirror = d['mirror']
    kw = dict(edges=d['edges'], bone_lengths=d['bone_targets'], root_depth=d['root_depth'],
              poses_rel=d['metro_crop'], box_size_mm=float(d['box_size_mm']))
    key = scale.replace('-', '_')
    for coords in OPL.COORDS:
        poses, kp, z = OPL.place(d['coords01'], q, int(d['stride']), scale, coords, perm, mirror, **kw)
        want = d[f'{key}_{coords}']
        scale_mm = np.abs(want).max(axis=(1, 2), keepdims=True)
        assert np.abs(poses - want).max() <= 1e-6 * scale_mm.max(), (coords, np.abs(poses - want).max())
        if scale != 'metro':
            assert np.allclose(z, d[f'{key}_z_offset'], rtol=1e-6)
    assert np.isfinite(kp).all()
    assert np.abs(kp - d['keypoints']).max() <= 1e-3, np.abs(kp - d['keypoints']).max()


def test_reference_fast_keypoint_path_is_inverted():
    """Recorded reference finding: reproject_image_points_fast (cameralib.py:432-438) maps the other way round; the fixture's
    keypoints come from the general branch.  For the undistorted camera the fast path's answer is far from them."""
    d = np.load(FIX)
    und = d['box_camera'] == 2
    assert np.abs(d['fast_keypoints'][und] - d['keypoints'][und]).max() > 100


@pytest.mark.parametrize('per_pose', [False, True])
def test_bone_lengths_round_trip_recovers_world_positions(per_pose):
    """Known answer: world poses seen by each virtual camera -> exact soft-argmax coordinates (no noise, exact bone lengths)
    -> the bone-length placement recovers the world positions to <= 1 mm."""
    d, q = fixture_params()
    fr = np.load(FRAMES_FIX)
    cams = fixture_cameras(fr)
    stride, side, box = int(d['stride']), int(d['side']), float(d['box_size_mm'])
    lrc = (side - 1) - ((side - 1) % stride) - 1
    rng = np.random.default_rng(7)
    base = np.array([[-130, 0, 0], [-140, 440, 30], [-150, 880, 0], [130, 0, 0], [140, 440, -20], [150, 880, 10],
                     [0, -230, 10], [0, -480, 0], [0, -560, -30], [0, -700, -10], [170, -450, 0], [260, -200, 40],
                     [300, 30, 80], [-170, -450, 0], [-270, -210, -30], [-320, 20, -60], [0, 0, 0]], np.float64)
    edges = np.asarray(SK.head_edges)
    bones = np.linalg.norm(base[edges[:, 0]] - base[edges[:, 1]], axis=1)
    c01, world = [], []
    for i in range(len(d['boxes'])):
        virt = look_at_box(cams[d['box_camera'][i]], d['boxes'][i], side)
        x = base + [rng.uniform(-200, 200), -150, rng.uniform(3000, 6000)]            # virtual-camera coordinates
        k = np.asarray(virt.intrinsic_matrix, np.float64)
        uv = x[:, :2] / x[:, 2:] @ k[:2, :2].T + k[:2, 2]
        c01.append(np.concatenate([(uv - stride // 2) / lrc, ((x[:, 2] - x[-1, 2]) / box + 0.5)[:, None]], 1))
        world.append(x @ virt.R.astype(np.float64) + virt.t)                            # R^T x + t
    c01 = np.asarray(c01, np.float32)
    world = np.asarray(world)[:, list(SK.permutation)]
    targets = np.tile(bones, (len(c01), 1)) if per_pose else bones
    poses, _, z = OPL.place(c01, q, stride, 'bone-lengths', 'world', SK.permutation, SK.out_mirror, edges=edges,
                            bone_lengths=targets, box_size_mm=box)
    assert np.abs(poses - world).max() <= 1.0, np.abs(poses - world).max()


def test_placement_struct_layout_matches_compiler(tmp_path):
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "metro_hip.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(MetroPlacement), offsetof(MetroPlacement, inv_intrinsics), '
                   'offsetof(MetroPlacement, rot_to_orig_cam), offsetof(MetroPlacement, rot_to_world), '
                   'offsetof(MetroPlacement, cam_loc), offsetof(MetroPlacement, homography), '
                   'offsetof(MetroPlacement, intrinsics), offsetof(MetroPlacement, distortion));return 0;}')
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    P = _lib.MetroPlacement
    assert got == [C.sizeof(P), P.inv_intrinsics.offset, P.rot_to_orig_cam.offset, P.rot_to_world.offset, P.cam_loc.offset,
                   P.homography.offset, P.intrinsics.offset, P.distortion.offset]
    assert got[0] == 208
    d, q = fixture_params()
    raw = pack_placements(q)
    assert raw.shape == (len(q.keypoint_mode), 208)
    rec = _lib.MetroPlacement.from_buffer_copy(raw[3].tobytes())
    assert list(rec.inv_intrinsics) == q.inv_intrinsics[3].ravel().tolist() and list(rec.cam_loc) == q.cam_loc[3].tolist()


@pytest.fixture(scope='module')
def model_path(tmp_path_factory):
    spec = ModelSpec(50, 32, 'h36m', base_width=8)
    path = str(tmp_path_factory.mktemp('placement') / 'm.npz')
    save_model(path, spec, synth.make_params(spec.arch, spec.n_head_channels, spec.base_width, seed=0))
    return path


def test_locate_poses_rejects_bad_arguments(model_path):
    frame = np.zeros((100, 120, 3), np.uint8)
    boxes = np.array([[10., 10., 40., 60.], [50., 20., 30., 50.]])
    cam = Camera(np.array([[500., 0, 60], [0, 500, 50], [0, 0, 1]]))
    e = len(SK.head_edges)
    call = lambda **kw: locate_poses_in_frames(frame, boxes, model_path, **kw)
    with pytest.raises(ValueError, match='needs calibrated cameras'):
        call(bone_lengths=np.full(e, 300.))
    with pytest.raises(ValueError, match='needs calibrated cameras'):
        call(scale_recovery='true-root-depth', root_depth=[4000., 4000.])
    with pytest.raises(ValueError, match='needs bone_lengths'):
        call(cameras=cam)
    with pytest.raises(ValueError, match=r'bone_lengths must be \[16\] or \[2, 16\]'):
        call(cameras=cam, bone_lengths=np.full(e + 1, 300.))
    with pytest.raises(ValueError, match=r'bone_lengths must be \[16\] or \[2, 16\]'):
        call(cameras=cam, bone_lengths=np.full((3, e), 300.))
    for bad in (0., -5., np.nan, np.inf):
        b = np.full(e, 300.)
        b[3] = bad
        with pytest.raises(ValueError, match='finite and positive'):
            call(cameras=cam, bone_lengths=b)
    with pytest.raises(ValueError, match=r'root_depth must be \[2\]'):
        call(cameras=cam, scale_recovery='true-root-depth', root_depth=[4000.])
    with pytest.raises(ValueError, match='finite and positive'):
        call(cameras=cam, scale_recovery='true-root-depth', root_depth=[4000., np.nan])
    with pytest.raises(ValueError, match='needs root_depth'):
        call(cameras=cam, scale_recovery='true-root-depth')
    with pytest.raises(ValueError, match='go with'):
        call(cameras=cam, scale_recovery='metro', bone_lengths=np.full(e, 300.))
    with pytest.raises(ValueError, match='scale_recovery must be'):
        call(cameras=cam, scale_recovery='bone-lengths-true')
    with pytest.raises(ValueError, match='coords must be'):
        call(cameras=cam, bone_lengths=np.full(e, 300.), coords='image')
    with pytest.raises(ValueError, match='boxes must be'):
        locate_poses_in_frames(frame, np.zeros((2, 3)), model_path, scale_recovery='metro')


def test_frozen_graph_skeleton_is_decoded_once_per_file(tmp_path, monkeypatch):
    """A .pb has no spec entry: its skeleton costs a whole decode, which happens once per (path, mtime), not once per call."""
    from metro_pose3d_amd import frames, modelfile, tfgraph
    spec = ModelSpec(50, 32, 'h36m', base_width=8)
    path = str(tmp_path / 'm.pb')
    tfgraph.write_frozen_graph(path, spec, synth.make_params(spec.arch, spec.n_head_channels, spec.base_width, seed=0))
    decodes = []
    real = modelfile.load_model
    monkeypatch.setattr(modelfile, 'load_model', lambda p: decodes.append(p) or real(p))
    frame = np.zeros((100, 120, 3), np.uint8)
    cam = Camera(np.array([[500., 0, 60], [0, 500, 50], [0, 0, 1]]))
    for _ in range(3):
        with pytest.raises(ValueError, match=r'bone_lengths must be \[16\]'):
            locate_poses_in_frames(frame, [[10., 10., 40., 60.]], path, cameras=cam, bone_lengths=np.full(5, 300.))
    assert len(decodes) == 1
    st = os.stat(path)
    os.utime(path, ns=(st.st_atime_ns, st.st_mtime_ns + 10**9))         # a rewritten file is read again
    with pytest.raises(ValueError, match=r'bone_lengths must be \[16\]'):
        locate_poses_in_frames(frame, [[10., 10., 40., 60.]], path, cameras=cam, bone_lengths=np.full(5, 300.))
    assert len(decodes) == 2 and frames._model_skeleton(path).n_head == 17 and len(decodes) == 2
