"""Test-time views of frame crops (frames.view_set / view_camera / view_params / pack_view_bases, metro_expand_views,
metro_merge_views): the new Camera methods and the view records against the reference's own camera code
(tests/golden/ref_views_v1.npz, made by tests/golden/make_ref_views.py), the view argument, the struct layouts, host work per
box rather than per view, and the NumPy merge on known answers.  No GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from metro_pose3d_amd import _lib, frames
from metro_pose3d_amd.frames import (Camera, estimate_pose_in_frames, euler2mat_ryxz, locate_poses_in_frames, look_at_box,
                                     pack_view_bases, view_camera, view_params, view_set)
from metro_pose3d_amd.joints import skeleton
from tests import oracle_views as OV
from tests.test_frames import fixture_cameras

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, 'tests', 'golden', 'ref_views_v1.npz')
FRAMES_FIX = os.path.join(ROOT, 'tests', 'golden', 'ref_frames_v1.npz')
SK = skeleton('h36m')


def fixture_views(d):
    return [(float(r), float(z), bool(f)) for r, z, f in zip(d['views_roll_deg'], d['views_zoom'], d['views_flip'])]


def _rx(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def _ry(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def _rz(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def test_euler2mat_ryxz_convention():
    """'ryxz' = Ry(yaw) Rx(pitch) Rz(roll); roll alone gives cos and sin exactly (what metro_expand_views is handed)."""
    rng = np.random.default_rng(3)
    for yaw, pitch, roll in rng.uniform(-3, 3, (20, 3)):
        assert np.allclose(euler2mat_ryxz(yaw, pitch, roll), _ry(yaw) @ _rx(pitch) @ _rz(roll), atol=1e-14)
    m = euler2mat_ryxz(0, 0, 0.3)
    assert m[0, 0] == math.cos(0.3) and m[1, 1] == math.cos(0.3) and m[1, 0] == math.sin(0.3) and m[0, 1] == -math.sin(0.3)
    assert (np.abs(m[2, :2]) == 0).all() and (np.abs(m[:2, 2]) == 0).all() and m[2, 2] == 1
    # a positive roll turns the camera counter-clockwise about its optical axis: image content turns clockwise
    cam = Camera(np.eye(3))
    cam.rotate(roll=math.pi / 2)
    assert np.allclose(cam.R @ [1, 0, 0], [0, -1, 0])


def test_camera_rotate_and_flip_match_the_reference():
    d, fr = np.load(FIX), np.load(FRAMES_FIX)
    cam0 = fixture_cameras(fr)[0]
    for (yaw, pitch, roll), want in zip(d['angles'], d['rotated_r']):
        cam = cam0.copy()
        cam.rotate(yaw=yaw, pitch=pitch, roll=roll)
        assert cam.R.dtype == np.float64
        assert np.abs(cam.R - want).max() <= 1e-12, (yaw, pitch, roll)
    cam = cam0.copy()
    cam.horizontal_flip()
    assert np.array_equal(cam.R, d['flipped_r']) and np.linalg.det(cam.R) < 0


def test_view_cameras_match_the_reference():
    """zoom, rotate(roll) and horizontal_flip applied to the reference's own look_at_box cameras (the frames fixture) give the
    reference's view cameras within 1e-12."""
    d, fr = np.load(FIX), np.load(FRAMES_FIX)
    k = 0
    for b in d['boxes']:
        virt = Camera(np.eye(3), R=fr['virt_r'][b])
        virt.intrinsic_matrix = np.asarray(fr['virt_k'][b], np.float64)
        for roll, zoom, flip in fixture_views(d):
            cam = view_camera(virt, roll, zoom, flip)
            assert np.abs(cam.intrinsic_matrix - d['view_k'][k]).max() <= 1e-12 * np.abs(d['view_k'][k]).max()
            assert np.abs(cam.R - d['view_r'][k]).max() <= 1e-12
            k += 1


def test_view_params_match_the_reference():
    """The host restatement of metro_expand_views (view_params) against the reference loader's rot_to_orig_cam, rot_to_world and
    inv(K) of every view (float32 like the loader's; our look_at_box agrees with the reference's to ~1e-7 relative)."""
    d, fr = np.load(FIX), np.load(FRAMES_FIX)
    boxes = fr['boxes'][d['boxes']]
    cams = fixture_cameras(fr)
    views = fixture_views(d)
    p, q = view_params(cams, boxes, fr['box_camera'][d['boxes']], views, int(d['side']))
    assert len(q.rot_to_orig_cam) == len(boxes) * len(views)
    assert np.abs(q.rot_to_orig_cam - d['rot_to_orig_cam']).max() <= 1e-6
    assert np.abs(q.rot_to_world - d['rot_to_world']).max() <= 1e-6
    rel = np.abs(q.inv_intrinsics - d['inv_k']) / np.abs(d['inv_k']).max(axis=(1, 2), keepdims=True)
    assert rel.max() <= 1e-6, rel.max()
    flipped = np.array([f for _, _, f in views] * len(boxes))
    assert ((np.linalg.det(q.rot_to_orig_cam.astype(np.float64)) < 0) == flipped).all()


def test_identity_view_keeps_the_records_of_the_box():
    fr = np.load(FRAMES_FIX)
    cams = fixture_cameras(fr)
    for cameras in (cams, None):
        p0, q0, _ = frames._frame_params_and_cameras(cameras, fr['boxes'], fr['box_camera'], 256)
        p, q = view_params(cameras, fr['boxes'], fr['box_camera'], [(0, 1, False), (5, 1, False)], 256)
        for a, b in zip(p0 + q0, p + q):
            assert np.array_equal(a, b[0::2])


def test_no_camera_views_are_similarities_about_the_crop_centre():
    """cameras=None: a view maps its crop pixel to the frame through the square crop's homography after the similarity
    p -> c + R(roll) F (p - c) / zoom about c = (side/2, side/2); the flip mirrors about x = side/2."""
    side = 256
    box = [40., 60., 100., 180.]
    h0 = frames.box_homography(box, side).astype(np.float64)
    p, q = view_params(None, [box], [0], [(30, 1.5, True)], side)
    a = math.radians(30)
    sim = np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]) @ np.diag([-1, 1]) / 1.5
    c = np.array([side / 2, side / 2])
    for u in ([0., 0.], [128., 128.], [255., 17.], [3., 250.]):
        base = c + sim @ (np.asarray(u) - c)
        w = h0 @ [*base, 1]
        g = p.homography[0].astype(np.float64) @ [*u, 1]
        assert np.allclose(g[:2] / g[2], w[:2] / w[2], atol=1e-3)
    assert (q.inv_intrinsics == 0).all() and np.linalg.det(q.rot_to_orig_cam[0]) < 0
    assert np.allclose(q.rot_to_orig_cam[0][:2, :2], (np.diag([-1, 1]) @ np.array([[math.cos(a), math.sin(a)],
                                                                                   [-math.sin(a), math.cos(a)]])).T, atol=1e-7)


def test_default_view_set():
    v = view_set(5)
    assert np.array_equal(v.roll_deg, [-20, -10, 0, 10, 20]) and (v.zoom == 1).all()
    assert v.flip.tolist() == [False, True, False, True, False]
    one = view_set(1)
    assert one.roll_deg.tolist() == [0] and one.zoom.tolist() == [1] and one.flip.tolist() == [False]
    assert len(view_set(32).zoom) == 32
    t = view_set([(3, 1.1, True), (-2.5, 0.9, np.bool_(False))])
    assert t.roll_deg.tolist() == [3, -2.5] and t.zoom.tolist() == [1.1, 0.9] and t.flip.tolist() == [True, False]


BAD_VIEWS = [0, 33, -1, True, 2.0, 'five', [], [(0, 1, False)] * 33, [(0, 1)], [(0, 1, False, 0)], [(np.nan, 1, False)],
             [(np.inf, 1, False)], [(0, 0, False)], [(0, -1, False)], [(0, np.nan, False)], [(0, np.inf, False)],
             [(0, 1, 1)], [(0, 1, 'yes')], [(0, 1, None)], [('3', 1, False)], [(True, 1, False)], [(0, True, False)], [5]]


@pytest.mark.parametrize('bad', BAD_VIEWS, ids=[repr(b)[:40] for b in BAD_VIEWS])
def test_views_are_validated(bad):
    with pytest.raises(ValueError, match='view'):
        view_set(bad)
    frame = np.zeros((100, 120, 3), np.uint8)
    # both calls check `views` before they touch the model file or a device
    with pytest.raises(ValueError, match='view'):
        estimate_pose_in_frames(frame, [[10., 10., 40., 60.]], 'no-such-model.npz', views=bad)
    with pytest.raises(ValueError, match='view'):
        locate_poses_in_frames(frame, [[10., 10., 40., 60.]], 'no-such-model.npz', scale_recovery='metro', views=bad)


def test_crop_coords_take_one_view():
    frame = np.zeros((100, 120, 3), np.uint8)
    for views in (2, [(0, 1, False), (0, 1, False)]):
        with pytest.raises(ValueError, match="coords='crop' takes one view"):
            estimate_pose_in_frames(frame, [[10., 10., 40., 60.]], 'no-such-model.npz', coords='crop', views=views)
        with pytest.raises(ValueError, match="coords='crop' takes one view"):
            locate_poses_in_frames(frame, [[10., 10., 40., 60.]], 'no-such-model.npz', scale_recovery='metro', coords='crop',
                                   views=views)


def test_view_struct_layouts_match_compiler(tmp_path):
    fields = ['frame', 'mode', 'has_camera', 'old_matrix', 'orig_r', 'virt_k', 'virt_r', 'partial', 'homography',
              'inv_intrinsics', 'rot_to_orig_cam', 'rot_to_world', 'cam_loc', 'intrinsics', 'distortion']
    vfields = ['cos_roll', 'sin_roll', 'zoom', 'flip']
    expr = ['sizeof(MetroViewBase)'] + [f'offsetof(MetroViewBase, {f})' for f in fields] + \
           ['sizeof(MetroView)'] + [f'offsetof(MetroView, {f})' for f in vfields] + ['(size_t)METRO_MAX_VIEWS']
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "metro_hip.h"\nint main(void){' +
                   ''.join(f'printf("%zu\\n", (size_t)({e}));' for e in expr) + 'return 0;}')
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    B, V = _lib.MetroViewBase, _lib.MetroView
    want = [C.sizeof(B)] + [getattr(B, f).offset for f in fields] + [C.sizeof(V)] + [getattr(V, f).offset for f in vfields] + \
           [_lib.METRO_MAX_VIEWS]
    assert got == want
    assert got[0] == 576 and got[len(fields) + 1] == 32
    assert frames.VIEW_BASE_DTYPE.itemsize == 576


def test_view_bases_hold_the_box_records():
    """pack_view_bases (column-wise, no per-record ctypes loop) against the ctypes packers of the records it embeds."""
    fr = np.load(FRAMES_FIX)
    cams = fixture_cameras(fr)
    p, q, virts = frames._frame_params_and_cameras(cams, fr['boxes'], fr['box_camera'], 256)
    raw = pack_view_bases(cams, fr['boxes'], fr['box_camera'], 256)
    crops = frames.pack_crops(p, fr['box_camera'])
    places = frames.pack_placements(q)
    for i in range(len(raw)):
        b = _lib.MetroViewBase.from_buffer_copy(raw[i].tobytes())
        c = _lib.MetroCropWarp.from_buffer_copy(crops[i].tobytes())
        pl = _lib.MetroPlacement.from_buffer_copy(places[i].tobytes())
        assert (b.frame, b.mode, b.has_camera) == (c.frame, c.mode, 1)
        for f in ('partial', 'homography', 'intrinsics', 'distortion'):
            assert list(getattr(b, f)) == list(getattr(c, f)), f
        for f in ('inv_intrinsics', 'rot_to_orig_cam', 'rot_to_world', 'cam_loc'):
            assert list(getattr(b, f)) == list(getattr(pl, f)), f
        orig = cams[fr['box_camera'][i]]
        assert list(b.virt_r) == virts[i].R.ravel().tolist() and list(b.virt_k) == virts[i].intrinsic_matrix.ravel().tolist()
        assert list(b.orig_r) == orig.R.ravel().tolist()
        assert list(b.old_matrix) == (orig.intrinsic_matrix @ orig.R).ravel().tolist()
    raw = pack_view_bases(None, fr['boxes'][:3], [0, 0, 0], 256)
    b = _lib.MetroViewBase.from_buffer_copy(raw[1].tobytes())
    assert b.has_camera == 0 and list(b.homography) == frames.box_homography(fr['boxes'][1], 256).ravel().tolist()


class _Stop(Exception):
    pass


@pytest.mark.parametrize('cameras', ['fixture', None])
def test_host_work_is_per_box_not_per_view(monkeypatch, cameras):
    """The chain's host phase (_warp_views up to the expansion launch): look_at_box and the record packing run once per
    box whatever V is, views=None included; no per-crop record is packed on the host (the device writes them)."""
    fr = np.load(FRAMES_FIX)
    cams = fixture_cameras(fr) if cameras else None
    calls = {'look_at_box': 0, 'pack_crops': 0, 'pack_placements': 0, 'bases_rows': []}

    def counting(name, fn):
        def wrapped(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return wrapped

    monkeypatch.setattr(frames, 'look_at_box', counting('look_at_box', look_at_box))
    monkeypatch.setattr(frames, 'pack_crops', counting('pack_crops', frames.pack_crops))
    monkeypatch.setattr(frames, 'pack_placements', counting('pack_placements', frames.pack_placements))
    monkeypatch.setattr(frames, '_device_frames', lambda f, device: [None] * 3)

    def stop(bases, vs, side, device):
        calls['bases_rows'].append((len(bases), len(vs.zoom), len(frames.view_table(vs))))
        raise _Stop

    monkeypatch.setattr(frames, '_expand_views', stop)
    n = len(fr['boxes'])
    for nv in (1, 5):
        calls['look_at_box'] = 0
        with pytest.raises(_Stop):
            frames._warp_views(None, cams, fr['boxes'], fr['box_camera'].astype(np.int64), view_set(nv), 256, None)
        assert calls['look_at_box'] == (n if cameras else 0)
        assert calls['bases_rows'][-1] == (n, nv, nv)
    assert calls['pack_crops'] == 0 and calls['pack_placements'] == 0
    # views=None is the same chain with the identity view: the public calls up to the expansion, the engine and the device
    # stubbed (no model file, no GPU)
    import contextlib
    import types

    import torch
    from metro_pose3d_amd import inference
    engine = types.SimpleNamespace(spec=types.SimpleNamespace(proc_side=256))
    monkeypatch.setattr(inference, '_engine_for', lambda *a, **kw: engine)
    monkeypatch.setattr(inference, '_resolve_device', lambda t: None)
    monkeypatch.setattr(torch.cuda, 'device', lambda device: contextlib.nullcontext())
    monkeypatch.setattr(frames, '_model_skeleton', lambda path: SK)
    frame = [np.zeros((8, 8, 3), np.uint8)] * 3
    for call in (lambda **kw: estimate_pose_in_frames(frame, fr['boxes'], 'no-such-model.npz', cameras=cams,
                                                      frame_index=fr['box_camera'], **kw),
                 lambda **kw: locate_poses_in_frames(frame, fr['boxes'], 'no-such-model.npz', cameras=cams,
                                                     frame_index=fr['box_camera'], scale_recovery='metro', **kw)):
        for views, nv in ((None, 1), (1, 1), (5, 5)):
            calls['look_at_box'] = 0
            with pytest.raises(_Stop):
                call(views=views)
            assert calls['look_at_box'] == (n if cameras else 0)
            assert calls['bases_rows'][-1] == (n, nv, nv)
    assert calls['pack_crops'] == 0 and calls['pack_placements'] == 0


# ---- the NumPy merge (tests/oracle_views.py) on known answers ----------------------------------------------------------------

def _flip_rot():
    return np.diag([-1., 1., 1.]).astype(np.float32)


def test_merge_known_answers():
    nj = SK.n_out
    mirror = np.asarray(SK.out_mirror)
    rng = np.random.default_rng(0)
    base = rng.normal(0, 300, (nj, 3)).astype(np.float32)
    kp = rng.uniform(0, 500, (nj, 2)).astype(np.float32)
    # two views: the first as is, the second offset by +-d and flipped (its keypoint labels are mirrored)
    d = np.array([10., -20., 5.], np.float32)
    poses = np.stack([base - d, base + d])
    kps = np.stack([kp, kp[mirror]])
    rots = np.stack([np.eye(3, dtype=np.float32), _flip_rot()])
    m, k, z, s = OV.merge(poses, kps, np.array([4000., 4100.], np.float32), rots, mirror, 2)
    assert np.allclose(m[0], base, atol=1e-4)
    assert np.array_equal(k[0], kp)                                  # the flipped view's mirror joint is the same point
    assert z.tolist() == [4050.]
    assert np.allclose(s[0], np.linalg.norm(d), rtol=1e-6)         # RMS distance of +-d from the mean


def test_merge_excludes_nan_keypoints_and_keeps_all_nan_joints_nan():
    nj = SK.n_out
    mirror = np.asarray(SK.out_mirror)
    poses = np.zeros((3, nj, 3), np.float32)
    kps = np.stack([np.full((nj, 2), 10.), np.full((nj, 2), 20.), np.full((nj, 2), 60.)]).astype(np.float32)
    kps[2, 4, 0] = np.nan                      # joint 4: view 2 excluded -> mean of 10 and 20
    kps[:, 7, 1] = np.nan                      # joint 7: no finite view -> NaN
    kps[1, 9] = np.inf                         # joint 9: view 1 excluded -> mean of 10 and 60
    rots = np.tile(np.eye(3, dtype=np.float32), (3, 1, 1))
    _, k, z, s = OV.merge(poses, kps, None, rots, mirror, 3)
    assert z is None and (s == 0).all()
    assert k[0, 0].tolist() == [30., 30.] and k[0, 4].tolist() == [15., 15.] and k[0, 9].tolist() == [35., 35.]
    assert np.isnan(k[0, 7]).all()


def test_merge_of_identical_views_is_exact():
    rng = np.random.default_rng(1)
    one = rng.normal(0, 500, (2, SK.n_out, 3)).astype(np.float32)
    kp = rng.uniform(0, 900, (2, SK.n_out, 2)).astype(np.float32)
    nv = 7
    rots = np.tile(np.eye(3, dtype=np.float32), (2 * nv, 1, 1))
    m, k, z, s = OV.merge(np.repeat(one, nv, axis=0), np.repeat(kp, nv, axis=0), np.repeat(np.float32([3000.5, 4000.25]), nv),
                          rots, SK.out_mirror, nv)
    assert np.array_equal(m, one) and np.array_equal(k, kp) and z.tolist() == [3000.5, 4000.25] and (s == 0).all()


def test_cli_views_flag(tmp_path, capsys):
    from metro_pose3d_amd import inference
    with pytest.raises(SystemExit):
        inference.main(['--model-path', 'm.npz', '--views', '5'])
    assert '--views go with --frame' in capsys.readouterr().err
    frame = tmp_path / 'f.npy'
    np.save(frame, np.zeros((100, 120, 3), np.uint8))
    with pytest.raises(SystemExit, match=r'views must lie in \[1, 32\]'):
        inference.main(['--model-path', 'no-such-model.npz', '--frame', str(frame), '--box', '10,10,40,60', '--views', '0'])
