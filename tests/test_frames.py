"""Frames in, poses out (metro_pose3d_amd/frames.py): the host geometry against the reference's own camera code
(tests/golden/ref_frames_v1.npz, made by tests/golden/make_ref_frames.py), known answers, and the new C entry's argument
checks.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from metro_pose3d_amd import _lib
from metro_pose3d_amd.frames import Camera, crop_params, look_at_box, undistort_points
from metro_pose3d_amd.joints import skeleton
from tests import oracle_frames as OP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, 'tests', 'golden', 'ref_frames_v1.npz')


def fixture_cameras(d):
    cams = []
    for i in range(3):
        dist = d[f'cam{i}_dist']
        cams.append(Camera(d[f'cam{i}_k'], dist if dist.size else None, d[f'cam{i}_r'], d[f'cam{i}_t'],
                           world_up=tuple(d[f'cam{i}_world_up'].tolist())))
    return cams


def test_look_at_box_matches_the_reference():
    d = np.load(FIX)
    cams = fixture_cameras(d)
    for i, (box, c) in enumerate(zip(d['boxes'], d['box_camera'])):
        virt = look_at_box(cams[c], box, int(d['side']))
        assert virt.intrinsic_matrix.dtype == np.float64 and virt.R.dtype == np.float32
        assert np.allclose(virt.intrinsic_matrix, d['virt_k'][i], rtol=1e-6, atol=0), i
        assert np.allclose(virt.R, d['virt_r'][i], rtol=1e-6, atol=1e-7), i
        cam = cams[c]
        k, r = OP.look_at_box(cam.intrinsic_matrix, cam.distortion_coeffs, cam.R, cam.t, cam.world_up, box, int(d['side']))
        assert np.allclose(k, d['virt_k'][i], rtol=1e-6, atol=0) and np.allclose(r, d['virt_r'][i], rtol=1e-6, atol=1e-7), i
    p = crop_params(cams, d['boxes'], d['box_camera'], int(d['side']))
    assert np.allclose(p.rot_to_orig_cam, d['rot_to_orig_cam'], atol=1e-6)
    assert np.allclose(p.rot_to_world, d['rot_to_world'], atol=1e-6)
    assert (p.mode == np.where(d['box_camera'] < 2, _lib.METRO_WARP_DISTORTED, _lib.METRO_WARP_HOMOGRAPHY)).all()


def test_warp_maps_match_the_reference():
    """The oracle's maps (which the HIP kernel reproduces to the byte on the GPU) against the maps the reference's own
    reproject_image hands to cv2.remap: bit for bit on >= 99.9 % of the coordinates, within one float32 ulp on the rest
    (NumPy's float64 matmul may sum the ray in another order)."""
    d = np.load(FIX)
    side, sub = int(d['side']), d['subgrid']
    p = crop_params(fixture_cameras(d), d['boxes'], d['box_camera'], side)
    same = total = 0
    for i in range(len(d['boxes'])):
        if p.mode[i] == _lib.METRO_WARP_DISTORTED:
            mx, my = OP.distorted_crop_coordinates(p.partial[i], p.intrinsics[i], p.distortion[i], side)
        else:
            mx, my = OP.crop_coordinates(p.homography[i], side)
        got = np.stack([mx, my])[:, sub][:, :, sub]
        ref = d['maps'][i]
        assert np.isfinite(ref).all() and np.isfinite(got).all()
        ulps = np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
        assert ulps.max() <= 1, (i, ulps.max())
        if p.mode[i] == _lib.METRO_WARP_HOMOGRAPHY:
            assert ulps.max() == 0, i                   # the same float32 matmul as the reference
        same += int((ulps == 0).sum())
        total += ulps.size
    assert same >= 0.999 * total, (same, total)


def test_undistort_points_known_answers():
    k = np.array([[1145., 0, 512.5], [0, 1143., 515.5], [0, 0, 1]], np.float32)
    pts = np.random.default_rng(0).uniform(-100, 1100, (200, 2)).astype(np.float32)
    got = undistort_points(pts, k, None)
    u, v = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    assert got.dtype == np.float32
    assert np.array_equal(got[:, 0], ((u - 512.5) * (1 / 1145.)).astype(np.float32))     # OpenCV multiplies by 1/fx
    assert np.array_equal(got[:, 1], ((v - 515.5) * (1 / 1143.)).astype(np.float32))
    assert np.abs(got[:, 0].astype(np.float64) - (u - 512.5) / 1145.).max() <= 1e-7
    assert np.array_equal(OP.undistort_points(pts, k, None), got)
    d = np.load(FIX)
    for i, cam in enumerate(fixture_cameras(d)[:2]):
        h, w = d[f'cam{i}_frame_hw']
        pts = np.random.default_rng(1).uniform([0, 0], [w, h], (2000, 2)).astype(np.float32)
        und = undistort_points(pts, cam.intrinsic_matrix, cam.distortion_coeffs)
        assert np.array_equal(und, OP.undistort_points(pts, cam.intrinsic_matrix, cam.distortion_coeffs))
        ray = np.concatenate([und, np.ones_like(und[:, :1])], 1)
        u, v = OP.project_points(ray, cam.intrinsic_matrix, cam.distortion_coeffs)
        err = np.abs(np.stack([u, v], 1) - pts).max(axis=1)
        radius = np.linalg.norm(pts - cam.intrinsic_matrix[:2, 2], axis=1)
        assert err[radius < 600].max() <= 1e-3
        # OpenCV's fixed five iterations have not converged in the corners of the strongly distorted 3DHP camera
        # (k1 = -0.28): up to ~0.05 px there
        assert err.max() <= (1e-3 if i == 0 else 0.1), (i, err.max())


def test_centred_box_on_an_intrinsics_only_camera_is_a_zoom():
    k = np.array([[1000., 0, 640], [0, 1000, 360], [0, 0, 1]])
    cam = Camera(k)
    assert cam.world_up.tolist() == [0, -1, 0] and Camera(k, R=np.eye(3)).world_up.tolist() == [0, 0, 1]
    virt = look_at_box(cam, (590, 260, 100, 200), 256)
    assert np.array_equal(virt.R, np.eye(3, dtype=np.float32))
    p = crop_params(cam, [(590, 260, 100, 200)], [0], 256)
    hom = p.homography[0].astype(np.float64)
    s = 200 / 256
    assert p.mode[0] == _lib.METRO_WARP_HOMOGRAPHY
    assert np.allclose(hom, [[s, 0, 640 - 128 * s], [0, s, 360 - 128 * s], [0, 0, 1]], rtol=1e-6, atol=1e-4)
    assert hom[0, 1] == hom[1, 0] == hom[2, 0] == hom[2, 1] == 0
    # any coefficient array, even zeros, takes the general mode (cameralib.py:272); None and no camera the homography mode
    assert crop_params(Camera(k, np.zeros(5)), [(590, 260, 100, 200)], [0], 256).mode[0] == _lib.METRO_WARP_DISTORTED
    q = crop_params(None, [(590, 260, 100, 200)], [0], 256)
    assert q.mode[0] == _lib.METRO_WARP_HOMOGRAPHY and (q.rot_to_orig_cam == np.eye(3)).all()


@pytest.mark.parametrize('dataset', ['h36m', 'many19', 'merged'])
def test_out_mirror_is_an_involution_on_output_joints(dataset):
    sk = skeleton(dataset)
    m = np.asarray(sk.out_mirror)
    assert m.shape == (sk.n_out,) and m.min() >= 0 and m.max() < sk.n_out
    assert (m[m] == np.arange(sk.n_out)).all()
    other = lambda n: ('r' + n[1:]) if n.startswith('l') else ('l' + n[1:]) if n.startswith('r') else n
    assert [sk.names[j] for j in m] == [other(n) for n in sk.names]


def test_rays_behind_the_camera_sample_the_border():
    """A general-mode ray with z <= 0 becomes a NaN coordinate; cv_round_x86(NaN) = INT_MIN, whose integer part saturates to
    -32768: both taps lie outside every frame (h, w <= 32767), so the pixel is the border value 0."""
    ang = np.deg2rad(80)
    ry = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    partial = ry @ np.linalg.inv(np.array([[100., 0, 32], [0, 100, 32], [0, 0, 1]]))
    k = np.array([[500., 0, 320], [0, 500, 240], [0, 0, 1]], np.float32)
    mx, my = OP.distorted_crop_coordinates(partial, k, np.float32([-0.2, 0.05, 0.001, -0.001, 0]), 64)
    behind = np.isnan(mx)
    assert behind.any() and not behind.all() and (np.isnan(my) == behind).all()
    frame = np.full((480, 640, 3), 200, np.uint8)
    out = OP.remap_u8_linear_constant0(frame, mx, my)
    assert (out[behind] == 0).all()
    assert OP.cv_round_x86(np.float32(np.nan) * 32) == -2 ** 31 and max(-32768, (-2 ** 31) >> 5) == -32768


def test_crop_frames_oracle_follows_the_mode():
    rng = np.random.default_rng(2)
    frames = [rng.integers(0, 256, (120, 160, 3), dtype=np.uint8), rng.integers(0, 256, (90, 70, 3), dtype=np.uint8)]
    hom = np.array([[1, 0, 3], [0, 1, 2], [0, 0, 1]], np.float32)
    k = np.array([[100., 0, 35], [0, 100, 45], [0, 0, 1]], np.float32)
    partial = np.linalg.inv(k.astype(np.float64))
    got = OP.crop_frames_u8(frames, [1, 0, 1], [0, 0, 1], np.stack([hom] * 3), np.stack([partial] * 3), np.stack([k] * 3),
                            np.zeros((3, 5), np.float32), 32)
    assert got.shape == (3, 32, 32, 3)
    assert np.array_equal(got[0], OP.reproject_image_fast(frames[1], hom, 32))
    assert np.array_equal(got[1], OP.reproject_image_fast(frames[0], hom, 32))
    assert np.array_equal(got[2], frames[1][:32, :32].astype(np.float32) / np.float32(255))   # zero distortion, K K^-1 = I


def test_crop_warp_struct_layout_matches_compiler(tmp_path):
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "metro_hip.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(MetroFrame), sizeof(MetroCropWarp), offsetof(MetroCropWarp, partial), '
                   'offsetof(MetroCropWarp, homography), offsetof(MetroCropWarp, intrinsics), offsetof(MetroCropWarp, distortion));'
                   'return 0;}')
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    w = _lib.MetroCropWarp
    assert got == [C.sizeof(_lib.MetroFrame), C.sizeof(w), w.partial.offset, w.homography.offset, w.intrinsics.offset,
                   w.distortion.offset] == [24, 160, 8, 80, 116, 140]


def test_warp_crops_frames_rejects_bad_arguments(lib):
    """Checked before any HIP call: no GPU needed."""
    p = C.c_void_p(256)
    out = C.c_void_p(512)

    def call(frames, n_frames=None, crops=p, n=1, side=16):
        tab = (_lib.MetroFrame * max(len(frames), 1))(*frames)
        return lib.metro_warp_crops_frames_u8(tab if frames else None, len(frames) if n_frames is None else n_frames,
                                              crops, n, side, out, None)

    ok = _lib.MetroFrame(256, 100, 120, 360, 0)
    for args, needle in (((([ok],), {'crops': None}), b'NULL'), ((([],), {}), b'NULL'),
                         ((([ok],), {'n_frames': 0}), b'frames'), ((([ok] * 65,), {}), b'65 frames'),
                         ((([ok],), {'n': 0}), b'bad geometry'), ((([ok],), {'side': 0}), b'bad geometry'),
                         ((([ok, _lib.MetroFrame(None, 100, 120, 360, 0)],), {}), b'frame 1: NULL'),
                         ((([_lib.MetroFrame(256, 100, 120, 359, 0)],), {}), b'stride'),
                         ((([_lib.MetroFrame(256, 32768, 120, 360, 0)],), {}), b'32767'),
                         ((([_lib.MetroFrame(256, 100, 1 << 30, 360, 0)],), {}), b'32767'),
                         ((([_lib.MetroFrame(256, 0, 120, 360, 0)],), {}), b'bad geometry')):
        assert call(*args[0], **args[1]) == -1, needle
        assert needle in lib.metro_last_error(), (needle, lib.metro_last_error())
