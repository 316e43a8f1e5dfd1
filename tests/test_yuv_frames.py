"""Frames in other pixel formats (metro_warp_crops_frames_planes, frames.py `pixel_format=` / `color_matrix=`): known answers
of the YUV rule (tests/oracle_yuv.py), its constants, the descriptor's layout, the C entry's argument checks and the Python
layout errors, all raised before any device work.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from metro_pose3d_amd import _lib
from metro_pose3d_amd import frames as FR
from metro_pose3d_amd.frames import COLOR_MATRICES, PIXEL_FORMATS
from tests import oracle_yuv as OY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rgb(y, u, v, matrix='bt601'):
    return OY.yuv420_to_rgb(np.full((2, 2), y, np.uint8), np.full((1, 1), u, np.uint8), np.full((1, 1), v, np.uint8),
                            matrix)[0, 0].tolist()


def test_the_formats_and_matrices():
    assert PIXEL_FORMATS == {'rgb': 0, 'bgr': 1, 'nv12': 2, 'i420': 3} and COLOR_MATRICES == {'bt601': 0, 'bt709': 1}
    assert set(OY.CONSTANTS) == set(COLOR_MATRICES)


@pytest.mark.parametrize('matrix', sorted(COLOR_MATRICES))
def test_known_answers_of_the_rule(matrix):
    assert _rgb(16, 128, 128, matrix) == [0, 0, 0]                  # limited-range black and white, neutral chroma
    assert _rgb(235, 128, 128, matrix) == [255, 255, 255]
    assert _rgb(126, 128, 128, matrix) == [128, 128, 128]           # (110 * CY + 2^19) >> 20
    # Y < 16 goes through max(0, Y - 16): Y = 0 and Y = 16 give the same colour, also where the chroma lifts it off 0
    for u, v in ((128, 128), (255, 255), (0, 255), (255, 0)):
        assert _rgb(0, u, v, matrix) == _rgb(16, u, v, matrix), (u, v)
    assert _rgb(0, 128, 255, matrix)[0] > 0
    # extreme chroma saturates each channel at both ends
    assert _rgb(235, 128, 255, matrix)[0] == 255 and _rgb(16, 128, 0, matrix)[0] == 0
    assert _rgb(235, 255, 128, matrix)[2] == 255 and _rgb(16, 0, 128, matrix)[2] == 0
    assert _rgb(235, 0, 0, matrix)[1] == 255 and _rgb(16, 255, 255, matrix)[1] == 0


def test_known_answers_against_the_formula():
    cy, cvr, cvg, cug, cub = OY.CONSTANTS['bt601']
    y, u, v = 100, 90, 200
    yy = (y - 16) * cy + (1 << 19)
    want = [(yy + cvr * (v - 128)) >> 20, (yy + cvg * (v - 128) + cug * (u - 128)) >> 20, (yy + cub * (u - 128)) >> 20]
    assert _rgb(y, u, v) == [min(max(c, 0), 255) for c in want] == [213, 54, 21]
    # floor shift, not truncation, for negative sums before the clamp: G of (Y 16, U 255, V 255) is far below 0
    assert _rgb(16, 255, 255)[1] == 0


def test_a_2x2_block_shares_one_chroma_pair():
    y = np.array([[16, 60, 100, 140], [180, 235, 30, 200]], np.uint8)
    u, v = np.array([[40, 220]], np.uint8), np.array([[200, 70]], np.uint8)
    rgb = OY.yuv420_to_rgb(y, u, v)
    for r in range(2):
        for c in range(4):
            assert rgb[r, c].tolist() == _rgb(y[r, c], u[0, c // 2], v[0, c // 2]), (r, c)


def test_the_constants_are_the_rounded_coefficients():
    for m in ('bt601', 'bt709'):
        assert OY.CONSTANTS[m] == tuple(int(round(c * (1 << 20))) for c in OY.COEFFICIENTS[m])
    assert OY.CONSTANTS['bt601'] == (1220542, 1673527, -852492, -409993, 2116026)       # OpenCV's ITUR_BT_601_C*
    # every intermediate of the rule fits in int32
    for m in ('bt601', 'bt709'):
        cy, cvr, cvg, cug, cub = OY.CONSTANTS[m]
        hi = 239 * cy + (1 << 19) + max(cvr * 127, cub * 127, -cvg * 128 - cug * 128)
        lo = (1 << 19) + min(-cvr * 128, -cub * 128, cvg * 127 + cug * 127)
        assert -(1 << 31) < lo and hi < (1 << 31)
    # the header states the same constants
    header = open(os.path.join(ROOT, 'include', 'metro_hip.h')).read()
    for m, name in (('bt601', 'METRO_YUV_BT601'), ('bt709', 'METRO_YUV_BT709')):
        line = next(ln for ln in header.splitlines() if name in ln and 'CY' in ln)
        assert [int(t) for t in line.split()[-9::2]] == list(OY.CONSTANTS[m]), line


def test_one_array_layouts_round_trip():
    y, u, v = OY.random_planes(6, 8, 0)
    for make, split in ((OY.nv12_frame, OY.nv12_planes), (OY.i420_frame, OY.i420_planes)):
        f = make(y, u, v)
        assert f.shape == (9, 8) and f.dtype == np.uint8
        assert all(np.array_equal(a, b) for a, b in zip(split(f), (y, u, v)))
    assert np.array_equal(OY.nv12_frame(y, u, v)[6], np.stack([u[0], v[0]], -1).reshape(-1))


def test_frame_planes_struct_layout_matches_compiler(tmp_path):
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "metro_hip.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(MetroFramePlanes), offsetof(MetroFramePlanes, plane), '
                   'offsetof(MetroFramePlanes, h), offsetof(MetroFramePlanes, w), offsetof(MetroFramePlanes, stride), '
                   'offsetof(MetroFramePlanes, format), offsetof(MetroFramePlanes, matrix));'
                   'printf("%d %d %d %d %d %d\\n", METRO_PIX_RGB, METRO_PIX_BGR, METRO_PIX_NV12, METRO_PIX_I420, '
                   'METRO_YUV_BT601, METRO_YUV_BT709);return 0;}')
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    s = _lib.MetroFramePlanes
    assert got[:7] == [C.sizeof(s), s.plane.offset, s.h.offset, s.w.offset, s.stride.offset, s.format.offset,
                       s.matrix.offset] == [48, 0, 24, 28, 32, 40, 44]
    assert got[7:] == [_lib.METRO_PIX_RGB, _lib.METRO_PIX_BGR, _lib.METRO_PIX_NV12, _lib.METRO_PIX_I420,
                       _lib.METRO_YUV_BT601, _lib.METRO_YUV_BT709]


def _desc(fmt, h=100, w=120, planes=(256, 512, 768), strides=None, matrix=0):
    if strides is None:
        strides = {0: (3 * w, 0), 1: (3 * w, 0), 2: (w, w), 3: (w, w // 2)}.get(fmt, (3 * w, w))
    d = _lib.MetroFramePlanes()
    d.plane[:] = [p or None for p in planes]
    d.h, d.w, d.format, d.matrix = h, w, fmt, matrix
    d.stride[:] = list(strides)
    return d


def test_warp_crops_frames_planes_rejects_bad_arguments(lib):
    """Every check returns -1 with its message before any HIP call: no GPU needed."""
    p, out = C.c_void_p(256), C.c_void_p(512)

    def call(frames, n_frames=None, crops=p, n=1, side=16):
        tab = (_lib.MetroFramePlanes * max(len(frames), 1))(*frames)
        return lib.metro_warp_crops_frames_planes(tab if frames else None, len(frames) if n_frames is None else n_frames,
                                                  crops, n, side, out, None)

    ok = [_desc(f) for f in range(4)] + [_desc(2, matrix=1), _desc(3, matrix=1)]
    nv12, i420 = _lib.METRO_PIX_NV12, _lib.METRO_PIX_I420
    cases = [
        ((ok,), {'crops': None}, b'NULL pointer'), (([],), {}, b'NULL pointer'),
        ((ok,), {'n_frames': 0}, b'frames'), (([ok[0]] * 65,), {}, b'65 frames'),
        ((ok,), {'n': 0}, b'bad geometry'), ((ok,), {'side': 0}, b'bad geometry'),
        (([ok[0], _desc(4)],), {}, b'frame 1: unknown pixel format 4'), (([_desc(-1)],), {}, b'unknown pixel format -1'),
        (([_desc(nv12, matrix=2)],), {}, b'unknown colour matrix 2'), (([_desc(0, matrix=-1)],), {}, b'colour matrix'),
        (([_desc(0, planes=(0, 512, 768))],), {}, b'frame 0: NULL plane 0'),
        (([_desc(1, planes=(0, 0, 0))],), {}, b'NULL plane 0'),
        (([_desc(nv12, planes=(256, 0, 768))],), {}, b'NULL plane 1'),
        (([_desc(nv12, planes=(0, 512, 768))],), {}, b'NULL plane 0'),
        (([_desc(i420, planes=(256, 512, 0))],), {}, b'NULL plane 2'),
        (([_desc(i420, planes=(256, 0, 768))],), {}, b'NULL plane 1'),
        (([_desc(nv12, h=101)],), {}, b'even h and w'), (([_desc(nv12, w=121, strides=(121, 121))],), {}, b'even h and w'),
        (([_desc(i420, h=99)],), {}, b'even h and w'), (([_desc(i420, w=119, strides=(119, 60))],), {}, b'even h and w'),
        (([_desc(0, h=0)],), {}, b'outside [1, 32767]'), (([_desc(nv12, w=0, strides=(0, 0))],), {}, b'outside [1, 32767]'),
        (([_desc(0, h=32768)],), {}, b'32767'), (([_desc(i420, w=32768, strides=(32768, 16384))],), {}, b'32767'),
        (([_desc(0, strides=(359, 0))],), {}, b'stride[0] 359 < 360'), (([_desc(1, strides=(359, 0))],), {}, b'stride[0]'),
        (([_desc(nv12, strides=(119, 120))],), {}, b'stride[0] 119 < 120'),
        (([_desc(i420, strides=(119, 60))],), {}, b'stride[0] 119 < 120'),
        (([_desc(nv12, strides=(120, 119))],), {}, b'stride[1] 119 < 120'),
        (([_desc(i420, strides=(120, 59))],), {}, b'stride[1] 59 < 60'),
    ]
    for args, kw, needle in cases:
        assert call(*args, **kw) == -1, needle
        assert needle in lib.metro_last_error(), (needle, lib.metro_last_error())


# ---- the Python layer: layout errors before any device work ----

def _nv12(h=6, w=8):
    return OY.nv12_frame(*OY.random_planes(h, w, 1))


def test_frame_set_accepts_the_layouts():
    y, u, v = OY.random_planes(6, 8, 2)
    for frames, fmt in ((_nv12(), 'nv12'), ((y, np.stack([u, v], -1)), 'nv12'), ((y, np.stack([u, v], -1).reshape(3, 8)), 'nv12'),
                        (OY.i420_frame(y, u, v), 'i420'), ((y, u, v), 'i420'), (np.zeros((6, 8, 3), np.uint8), 'bgr'),
                        ([torch.from_numpy(_nv12()), (y, np.stack([u, v], -1))], 'nv12')):
        fs = FR._frame_set(frames, fmt)
        assert isinstance(fs, FR._FrameSet) and len(fs.items) == (2 if isinstance(frames, list) else 1)
        for k, f in enumerate(fs.items):
            pl = FR._planar(k, f, fmt, 'bt601')
            assert (pl.h, pl.w) == (6, 8) and pl.format == FR.PIXEL_FORMATS[fmt]
    # the planes of a pitched NV12 array: the views and the array's row stride, no copy
    pitched = np.zeros((9, 16), np.uint8)[:, :8]
    pl = FR._planar(0, pitched, 'nv12', 'bt709')
    assert pl.stride == (16, 16) and pl.matrix == _lib.METRO_YUV_BT709 and pl.planes[1].shape == (3, 8)
    assert pl.planes[1].data_ptr() == torch.from_numpy(pitched).data_ptr() + 6 * 16
    pl = FR._planar(0, OY.i420_frame(y, u, v), 'i420', 'bt601')
    assert pl.stride == (8, 4) and [p.shape for p in pl.planes] == [(6, 8), (3, 4), (3, 4)]
    assert np.array_equal(pl.planes[1].numpy(), u) and np.array_equal(pl.planes[2].numpy(), v)
    # 'rgb' frames come back untouched: the unchanged metro_warp_crops_frames_u8 path
    rgb = [np.zeros((6, 8, 3), np.uint8)]
    assert FR._frame_set(rgb) is rgb and FR._frame_set(rgb, 'rgb', 'bt601') is rgb


def test_frame_set_rejects_bad_layouts():
    y, u, v = OY.random_planes(6, 8, 3)
    uv = np.stack([u, v], -1)
    bad = [
        ('nv12', np.zeros((6, 8, 3), np.uint8), r'frame 0: the frame is torch.uint8 \(6, 8, 3\)'),
        ('nv12', np.zeros((10, 8), np.uint8), r'10 rows are not H\*3/2'),
        ('nv12', np.zeros((9, 7), np.uint8), 'even height and width'),
        ('nv12', np.zeros((9, 8), np.float32), 'float32'),
        ('nv12', np.zeros((9, 16), np.uint8)[:, ::2], 'strides'),
        ('nv12', torch.zeros((8, 9), dtype=torch.uint8).t(), 'strides'),
        ('nv12', (y,), 'a tuple of 1 planes'),
        ('nv12', (y, u), r'the UV plane is \(3, 4\)'),
        ('nv12', (y, np.zeros((3, 4, 2, 1), np.uint8)), r'the UV plane is \(3, 4, 2, 1\)'),
        ('nv12', (y, np.ascontiguousarray(uv.transpose(2, 0, 1)).transpose(1, 2, 0)), 'strides'),
        ('nv12', (y[:, :7], uv), 'even height and width'),
        ('i420', np.zeros((9, 16), np.uint8)[:, :8], 'the frame has strides'),
        ('i420', (y, u), 'a tuple of 2 planes'),
        ('i420', (y, u, v[:, :3]), r'the U and V planes are \(3, 4\) and \(3, 3\)'),
        ('i420', (y, u, np.zeros((3, 8), np.uint8)[:, :4]), 'row strides 4 and 8'),
        ('bgr', np.zeros((6, 8, 4), np.uint8), r'the frame is \(6, 8, 4\)'),
        ('bgr', np.zeros((6, 8), np.uint8), r'frame 0: the frame is torch.uint8 \(8,\)'),     # a stack of 6 frames
    ]
    for fmt, frames, msg in bad:
        with pytest.raises(ValueError, match=msg):
            FR._frame_set(frames, fmt)
    with pytest.raises(ValueError, match=r"frame 1: .*pixel_format='nv12' takes a uint8 \[H\*3/2, W\]"):
        FR._frame_set([_nv12(), np.zeros((10, 8), np.uint8)], 'nv12')
    with pytest.raises(ValueError, match='65 frames'):
        FR._frame_set([_nv12()] * 65, 'nv12')
    with pytest.raises(ValueError, match='no frames'):
        FR._frame_set([], 'i420')
    with pytest.raises(ValueError, match='pixel_format must be'):
        FR._frame_set(_nv12(), 'yuyv')
    with pytest.raises(ValueError, match='color_matrix must be'):
        FR._frame_set(_nv12(), 'nv12', 'bt2020')
    for fmt in ('rgb', 'bgr'):
        with pytest.raises(ValueError, match="applies to 'nv12' and 'i420'"):
            FR._frame_set(np.zeros((6, 8, 3), np.uint8), fmt, 'bt709')


def test_public_calls_raise_layout_errors_before_device_work(monkeypatch):
    """The checks run first: no model is read, no device is touched (a missing model file and no GPU needed)."""
    from metro_pose3d_amd import inference
    touched = []
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: touched.append('current_device') or 0)
    monkeypatch.setattr(inference, '_engine_for', lambda *a, **k: touched.append('_engine_for'))
    boxes = np.array([[0.0, 0, 4, 4]])
    odd = np.zeros((9, 7), np.uint8)
    p = FR.crop_params(None, boxes, np.zeros(1), 16)
    calls = [lambda **kw: FR.estimate_pose_in_frames(odd, boxes, 'no-such-model.npz', **kw),
             lambda **kw: FR.estimate_pose_in_frames(odd, boxes, 'no-such-model.npz', views=5, **kw),
             lambda **kw: FR.estimate_pose_in_frames(odd, boxes, 'no-such-model.npz', geometry='device', **kw),
             lambda **kw: FR.locate_poses_in_frames(odd, boxes, 'no-such-model.npz', scale_recovery='metro', **kw),
             lambda **kw: FR.warp_frames(odd, p, np.zeros(1), 16, **kw)]
    for call in calls:
        with pytest.raises(ValueError, match='even height and width'):
            call(pixel_format='nv12')
        with pytest.raises(ValueError, match='color_matrix'):
            call(pixel_format='bgr', color_matrix='bt709')
    assert touched == []


def test_cli_pixel_format_flags(tmp_path, capsys):
    from metro_pose3d_amd import inference
    with pytest.raises(SystemExit):
        inference.main(['--model-path', 'm.npz', '--pixel-format', 'nv12'])
    assert '--pixel-format and --color-matrix go with --frame' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        inference.main(['--model-path', 'm.npz', '--frame', 'f.npy', '--pixel-format', 'yuyv'])
    assert 'invalid choice' in capsys.readouterr().err
    frame = tmp_path / 'f.npy'
    np.save(frame, np.zeros((100, 120, 3), np.uint8))          # an RGB frame read as NV12
    with pytest.raises(SystemExit, match=r"frame 0: the frame is torch.uint8 \(100, 120, 3\); pixel_format='nv12'"):
        inference.main(['--model-path', 'no-such-model.npz', '--frame', str(frame), '--box', '10,10,40,60',
                        '--pixel-format', 'nv12'])
    with pytest.raises(SystemExit, match="applies to 'nv12' and 'i420'"):
        inference.main(['--model-path', 'no-such-model.npz', '--frame', str(frame), '--box', '10,10,40,60',
                        '--color-matrix', 'bt709'])
    np.save(frame, np.zeros((150, 121), np.uint8))
    with pytest.raises(SystemExit, match='even height and width'):
        inference.main(['--model-path', 'no-such-model.npz', '--frame', str(frame), '--box', '10,10,40,60',
                        '--pixel-format', 'i420', '--intrinsics', '100,100,60,50', '--root-depth', '4000'])
