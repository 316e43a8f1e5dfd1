"""Crop geometry on the device (metro_look_at_boxes, frames.pack_frame_cameras, `geometry=`) without a GPU: the new record and
prototype against the compiler, the camera table against the Camera fields, the keyword's checks, and the kernel's arithmetic,
compiled for the host from the same source, against pack_view_bases."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from metro_pose3d_amd import _lib, frames as FR
from metro_pose3d_amd.frames import Camera, estimate_pose_in_frames, locate_poses_in_frames, pack_frame_cameras
from tests.test_frames import FIX, fixture_cameras
from tests.helpers import compile_for_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_frame_camera_layout_and_prototype_match_compiler(tmp_path):
    fields = ['intrinsics', 'r', 'r_inv', 't', 'distortion', 'has_distortion', 'world_up', 'old_matrix']
    expr = ['sizeof(MetroFrameCamera)'] + [f'offsetof(MetroFrameCamera, {f})' for f in fields]
    proto = ('int (*fn)(const double*, const int32_t*, int32_t, int32_t, const MetroFrameCamera*, int32_t, int32_t, '
             'MetroViewBase*, int32_t*, void*) = metro_look_at_boxes; (void)fn;')
    inc = os.path.join(ROOT, 'include')
    check = tmp_path / 'prototype.c'            # compiled only: a prototype that differs is an incompatible-pointer error
    check.write_text('#include "metro_hip.h"\nvoid f(void){' + proto + '}')
    subprocess.check_call(['gcc', '-std=c99', '-Werror', '-c', '-I', inc, str(check), '-o', str(tmp_path / 'prototype.o')])
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "metro_hip.h"\nint main(void){' +
                   ''.join(f'printf("%zu\\n", (size_t)({e}));' for e in expr) + 'return 0;}')
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-std=c99', '-I', inc, str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    S = _lib.MetroFrameCamera
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in fields]
    assert got[0] == 240 and FR.FRAME_CAMERA_DTYPE.itemsize == 240
    res, args = _lib.SIGNATURES['metro_look_at_boxes']
    assert res is C.c_int and len(args) == 10


def test_camera_table_holds_the_camera_fields():
    d = np.load(FIX)
    cams = fixture_cameras(d)
    plain = Camera(np.array([[1200., 0, 640], [0, 1180, 360], [0, 0, 1]]))        # intrinsics only, no distortion
    rec = pack_frame_cameras(cams + [plain], 4)
    assert len(rec) == 4 and rec.dtype == FR.FRAME_CAMERA_DTYPE
    for e, c in zip(rec, cams + [plain]):
        assert np.array_equal(e['intrinsics'], c.intrinsic_matrix.ravel())
        assert np.array_equal(e['r'], c.R.ravel()) and np.array_equal(e['t'], c.t)
        assert np.array_equal(e['r_inv'], np.linalg.inv(c.R).ravel())                  # camera_to_world's matrix
        assert np.array_equal(e['old_matrix'], (c.intrinsic_matrix @ c.R).astype(np.float64).ravel())
        assert np.array_equal(e['world_up'], np.asarray(c.world_up, np.float64))
        assert e['has_distortion'] == int(c.distortion_coeffs is not None)
        assert np.array_equal(e['distortion'], np.zeros(5) if c.distortion_coeffs is None else c.distortion_coeffs)
    assert rec[2]['has_distortion'] == 0 and rec[0]['has_distortion'] == 1          # the fixture's camera 2 has none
    assert list(rec[3]['world_up']) == [0, -1, 0] and list(rec[0]['world_up']) == list(d['cam0_world_up'])
    assert np.array_equal(rec[3]['r'].reshape(3, 3), np.eye(3)) and not rec[3]['t'].any()
    one = pack_frame_cameras(cams[1], 7)                                                 # one camera for every frame
    assert len(one) == 1 and np.array_equal(one[0]['r'], cams[1].R.ravel())
    assert len(pack_frame_cameras(cams, 2)) == 2                                         # the first n_frames of a list
    with pytest.raises(ValueError, match='3 Camera objects for 4 frames'):
        pack_frame_cameras(cams, 4)
    with pytest.raises(ValueError, match='frames.Camera'):
        pack_frame_cameras([cams[0], 'camera'], 2)


def test_geometry_rejects_bad_values_before_any_device_work():
    frames = np.zeros((8, 8, 3), np.uint8)
    for bad in ('gpu', 'Device', '', None, 1):
        with pytest.raises(ValueError, match='geometry must be'):
            estimate_pose_in_frames(frames, [[0, 0, 4, 4]], 'no-such-model.npz', geometry=bad)
        with pytest.raises(ValueError, match='geometry must be'):
            locate_poses_in_frames(frames, [[0, 0, 4, 4]], 'no-such-model.npz', scale_recovery='metro', geometry=bad)
    assert FR._geometry_of('auto', np.zeros((1, 4))) == 'host'
    assert FR._geometry_of('device', np.zeros((1, 4))) == 'device'


def test_kernel_arithmetic_on_the_host_matches_pack_view_bases(tmp_path):
    """look_at_boxes.hip's per-box functions are __host__ __device__: compiled for the host from the same source, they are held
    to the bounds the GPU test holds the kernel to (fp32 fields within 4 column-scaled ulp, fp64 fields within 1e-6
    column-scaled, cameras=None bit-identical), on the fixture's cameras and boxes inside, across and outside the frame."""
    lib = compile_for_host(tmp_path, 'host_look_at_boxes', ['look_at_boxes.hip'], '''
extern "C" void host_look_at_boxes(const double* boxes, const int32_t* fi, int n, const MetroFrameCamera* cams, int n_cameras,
                                   int side, MetroViewBase* out) {
    for (int i = 0; i < n; ++i) {
        out[i].frame = fi[i];
        out[i].reserved = 0;
        if (!cams) metro::square_crop_record(boxes + 4 * i, side, out[i]);
        else metro::camera_record(boxes + 4 * i, cams[n_cameras == 1 ? 0 : fi[i]], side, out[i]);
    }
}
''')
    d = np.load(FIX)
    boxes = np.concatenate([d['boxes'], [[-4000, 200, 300, 400], [1300, 1300, 150, 200], [-900, -900, 300, 300],
                                         [100, 100, 50, 400], [100, 100, 600, 80]]])
    fi = np.concatenate([d['box_camera'], [2, 0, 1, 0, 1]]).astype(np.int64)
    n = len(boxes)
    for variant in range(3):
        cams = fixture_cameras(d)
        if variant == 1:
            cams[2].distortion_coeffs = np.zeros(5, np.float32)
        if variant == 2:
            for c in cams:
                c.distortion_coeffs = None
        for cameras in (cams, cams[1], None):
            want = np.frombuffer(FR.pack_view_bases(cameras, boxes, fi, 256).tobytes(), FR.VIEW_BASE_DTYPE)
            got = np.zeros(n, FR.VIEW_BASE_DTYPE)
            table = None if cameras is None else pack_frame_cameras(cameras, 3)
            b, f = np.ascontiguousarray(boxes), np.ascontiguousarray(fi, np.int32)
            lib.host_look_at_boxes(C.c_void_p(b.ctypes.data), C.c_void_p(f.ctypes.data), n,
                                   None if table is None else C.c_void_p(table.ctypes.data), 0 if table is None else len(table),
                                   256, C.c_void_p(got.ctypes.data))
            if cameras is None:
                assert got.tobytes() == want.tobytes()
                continue
            for name in FR.VIEW_BASE_DTYPE.names:
                g, w = got[name].reshape(n, -1), want[name].reshape(n, -1)
                if g.dtype.kind == 'i' or name == 'orig_r':
                    assert (g == w).all(), name
                    continue
                scale = np.maximum(np.abs(g), np.abs(w))
                if g.shape[1] == 9:
                    scale = np.tile(scale.reshape(n, 3, 3).max(axis=1), (1, 3))
                if g.dtype == np.float32 or name == 'virt_r':
                    u = np.abs(g.astype(np.float64) - w) / np.spacing(scale.astype(np.float32)).astype(np.float64)
                    assert u.max() <= 4, (variant, name, u.max())
                else:
                    assert (np.abs(g - w) / np.where(scale > 0, scale, 1)).max() <= 1e-6, (variant, name)
