"""uint8 crops on the MI355X: every uint8 result must have the bits of the float32 path on np.float32(b) / np.float32(255).
Stem kernels, the conversion entry, the forward in three precisions, the byte-output warps and the frames chain; every
comparison is torch.equal / np.array_equal on raw values, no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

from metro_pose3d_amd import ModelSpec, _lib, save_model, synth
from metro_pose3d_amd import frames as FR
from metro_pose3d_amd.camera import Camera
from metro_pose3d_amd.engine import Engine
from metro_pose3d_amd.frames import crop_params, estimate_pose_in_frames, locate_poses_in_frames, warp_frames
from tests import helpers as H

pytestmark = pytest.mark.gpu
check = _lib.check


def _unit(u8: np.ndarray) -> np.ndarray:
    """The float32 image uint8 crops stand for."""
    return u8.astype(np.float32) / np.float32(255)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _crops(n, side, seed):
    """Random bytes with: every value 0..255 in each channel of crop 0 (A: the whole domain of the conversion); the first and
    last two rows and columns 255 (B: a wrong border or row clamp shows); an all-zero and an all-255 crop where n allows (C)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (n, side, side, 3), dtype=np.uint8)
    ramp = np.arange(side * side, dtype=np.int64)
    for c in range(3):
        img[0, :, :, c] = ((ramp * (2 * c + 1) + 85 * c) % 256).reshape(side, side).astype(np.uint8)      # odd step: all 256 values
        assert len(np.unique(img[0, :, :, c])) == 256
    img[:, :2] = 255; img[:, -2:] = 255; img[:, :, :2] = 255; img[:, :, -2:] = 255
    if n >= 2:
        img[n - 1] = 255
    if n >= 3:
        img[n - 2] = 0
    return img


@pytest.mark.parametrize('n,side', [(1, 256), (3, 256), (2, 96)])
def test_stem_u8in_has_the_bits_of_f32in(lib, cuda, n, side):
    u8 = _crops(n, side, seed=n * 1000 + side)
    rng = np.random.default_rng(5)
    wp = np.zeros((64, 7, 8, 4), np.float16)
    wp[:, :, :7, :3] = (rng.standard_normal((64, 7, 7, 3)) * np.sqrt(2.0 / 147)).astype(np.float16)
    tw = torch.from_numpy(wp).to(cuda)
    tb = torch.from_numpy((rng.standard_normal(64) * 0.5).astype(np.float32)).to(cuda)
    t8, t32 = torch.from_numpy(u8).to(cuda), torch.from_numpy(_unit(u8)).to(cuda)
    want = torch.full((n, side // 4, side // 4, 64), float('nan'), dtype=torch.float16, device=cuda)
    got = torch.full_like(want, float('nan'))
    lib.metro_kernel_notes(1)
    try:
        check(lib.metro_stem_pool_f32in(H.ptr(t32), H.ptr(tw), H.ptr(tb), H.ptr(want), n, side, None), 'metro_stem_pool_f32in')
        check(lib.metro_stem_pool_u8in(H.ptr(t8), H.ptr(tw), H.ptr(tb), H.ptr(got), n, side, None), 'metro_stem_pool_u8in')
        ids = lib.metro_last_kernel_id().decode()
    finally:
        lib.metro_kernel_notes(0)
    torch.cuda.synchronize()
    assert ('<rows,u8in>' in ids) == (side == 256) and ',u8in>' in ids and ',f32in>' in ids, ids
    assert torch.isfinite(want).all()
    assert torch.equal(_bits(got), _bits(want)), f'{(got != want).sum().item()} of {got.numel()} values differ ({ids})'


def test_images_u8_to_f32_is_numpys_division(lib, cuda):
    u8 = np.tile(np.arange(256, dtype=np.uint8), 3)
    u8 = np.concatenate([u8, u8[:1]])                         # 3 * 256 + 1: an odd length, more than one block
    t8 = torch.from_numpy(u8).to(cuda)
    out = torch.full((len(u8) + 1,), float('nan'), dtype=torch.float32, device=cuda)
    check(lib.metro_images_u8_to_f32(H.ptr(t8), len(u8), H.ptr(out), None), 'metro_images_u8_to_f32')
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:-1].view(np.uint32), _unit(u8).view(np.uint32))
    assert np.isnan(got[-1])                                  # nothing written past count


@pytest.fixture(scope='module')
def toy(tmp_path_factory):
    spec = ModelSpec(50, 32, 'h36m', base_width=8)
    params = synth.make_params(50, spec.n_head_channels, 8, seed=1, logit_gain=0.84)
    path = str(tmp_path_factory.mktemp('u8') / 'toy.npz')
    save_model(path, spec, params)
    return spec, params, path


@pytest.mark.parametrize('precision', ['f16', 'f32m', 'f64'])
def test_forward_u8_has_the_bits_of_the_float32_forward(cuda, toy, precision):
    """estimate_pose and Engine.forward (poses and coords01) at n = 1, n = 9 (past the 8-crop engine) and a sliced view."""
    from metro_pose3d_amd import inference as INF
    spec, params, path = toy
    u8 = _crops(10, spec.proc_side, seed=3)
    t8, t32 = torch.from_numpy(u8).to(cuda), torch.from_numpy(_unit(u8)).to(cuda)
    for what, sl in (('n=1', slice(0, 1)), ('n=9', slice(0, 9)), ('view [1:]', slice(1, 10))):
        want = INF.estimate_pose(t32[sl], path, precision=precision)[0]
        got = INF.estimate_pose(t8[sl], path, precision=precision)[0]
        assert torch.isfinite(want).all()
        assert torch.equal(_bits(got), _bits(want)), (precision, what)
        host = INF.estimate_pose(u8[sl], path, precision=precision)[0]          # a NumPy array of bytes from the host
        assert torch.equal(_bits(host), _bits(want)), (precision, what, 'host')
    eng = Engine(spec, params, precision, max_batch=16, device=cuda)
    sk = spec.skeleton
    for sl in (slice(0, 1), slice(0, 9), slice(1, 10)):
        n = sl.stop - sl.start
        c_want = torch.full((n, sk.n_head, 3), float('nan'), dtype=torch.float32, device=cuda)
        c_got = torch.full_like(c_want, float('nan'))
        p_want = eng.forward(t32[sl], coords01=c_want).clone()
        s_want = eng.status_words(n).clone()
        p_got = eng.forward(t8[sl], coords01=c_got)
        assert torch.equal(_bits(p_got), _bits(p_want)) and torch.equal(_bits(c_got), _bits(c_want)), (precision, sl)
        assert torch.equal(eng.status_words(n), s_want) and torch.isfinite(c_want).all()
        assert torch.equal(_bits(eng.forward(t8[sl])), _bits(p_want))             # without coords01: the same poses
    # a view that does not start on a 16-byte boundary is copied once, not refused
    flat = torch.zeros(u8[:2].size + 1, dtype=torch.uint8, device=cuda)
    flat[1:] = t8[:2].reshape(-1)
    odd = flat[1:].view(2, spec.proc_side, spec.proc_side, 3)
    assert odd.data_ptr() % 16 == 1
    assert torch.equal(_bits(eng.forward(odd)), _bits(eng.forward(t32[:2])))
    for bad in (torch.int8, torch.float64, torch.float16):
        with pytest.raises(ValueError):
            eng.forward(t8[:1].to(bad))
    eng.close()


def test_forward_u8_on_the_product_stem(cuda):
    """The full-width network at side 256: the forward whose first launch is stem_pool_f16<rows,u8in>."""
    spec = ModelSpec(50, 32, 'h36m')
    params = synth.make_params(50, spec.n_head_channels, 64, seed=2, logit_gain=synth.logit_gain_for(50, 32))
    eng = Engine(spec, params, 'f16', max_batch=4, device=cuda)
    assert any('rows,f32in' in k for k in eng.layer_kernels(3))
    u8 = _crops(3, 256, seed=11)
    want = eng.forward(torch.from_numpy(_unit(u8)).to(cuda)).clone()
    got = eng.forward(torch.from_numpy(u8).to(cuda))
    assert torch.isfinite(want).all() and torch.equal(_bits(got), _bits(want))
    eng.check_finite(3)
    eng.close()


def test_fp16_overflow_is_reported_for_uint8_crops_too(cuda):
    """synth.make_params(res_gain=3.0) on ResNet-101 overflows fp16 (tests/test_gpu_forward.py): the status words of a uint8
    call are those of the float32 call and check_finite raises alike."""
    spec = ModelSpec(101, 32, 'h36m')
    params = synth.make_params(101, spec.n_head_channels, 64, seed=0, logit_gain=1e-6, res_gain=3.0)
    eng = Engine(spec, params, 'f16', max_batch=2, device=cuda)
    u8 = (synth.make_images(2) * 255).astype(np.uint8)
    eng.forward(torch.from_numpy(_unit(u8)).to(cuda))
    words = eng.status_words(2).clone()
    with pytest.raises(_lib.NonFiniteError, match='f32m'):
        eng.check_finite(2)
    eng.forward(torch.from_numpy(u8).to(cuda))
    assert torch.equal(eng.status_words(2), words) and words.ne(0).any()
    with pytest.raises(_lib.NonFiniteError, match='f32m'):
        eng.check_finite(2)
    eng.close()


# ---- the warps ------------------------------------------------------------------------------------------------------

def _warp_scene(distorted):
    """Two frames of 64 x 48 and 37 x 53 (width x height) and three boxes: one inside frame 0, one partly outside frame 1,
    one on frame 0 again (its record gets an out-of-range frame index at the C level)."""
    rng = np.random.default_rng(21)
    frames = [rng.integers(0, 256, (48, 64, 3), dtype=np.uint8), rng.integers(0, 256, (53, 37, 3), dtype=np.uint8)]
    dist = [np.array([-0.2, 0.05, 0.001, -0.002, 0.01], np.float32), np.array([0.1, -0.03, 0.0, 0.001, 0.0], np.float32)]
    cams = [Camera(np.array([[60., 0, 32], [0, 60., 24], [0, 0, 1]]), dist[0] if distorted else None),
            Camera(np.array([[45., 0, 18], [0, 45., 26], [0, 0, 1]]), dist[1] if distorted else None)]
    boxes = np.array([[10., 8., 30., 30.], [20., 30., 30., 40.], [2., 2., 50., 40.]])
    fi = np.array([0, 1, 0])
    return frames, cams, boxes, fi


def _assert_bytes_are_the_float_crops(f32: torch.Tensor, u8: torch.Tensor, what):
    f32, u8 = f32.cpu().numpy(), u8.cpu().numpy()
    assert u8.dtype == np.uint8 and f32.dtype == np.float32 and u8.shape == f32.shape
    assert np.array_equal(f32.view(np.uint32), _unit(u8).view(np.uint32)), what


@pytest.mark.parametrize('side', [256, 33])
@pytest.mark.parametrize('distorted', [False, True])
def test_warp_bytes_are_the_float_crops(cuda, side, distorted):
    frames, cams, boxes, fi = _warp_scene(distorted)
    p = crop_params(cams, boxes, fi, side)
    assert (p.mode == int(distorted)).all()
    # the public call
    f32 = warp_frames(frames, p, fi, side, device=cuda)
    u8 = warp_frames(frames, p, fi, side, device=cuda, crop_dtype='uint8')
    _assert_bytes_are_the_float_crops(f32, u8, 'warp_frames')
    assert 0 < (u8 == 0).float().mean().item() < 1               # the box partly outside its frame met the border
    # the launches, with a frame index outside the table in the third record: zeros in both forms
    bad = np.array([0, 1, 2])
    recs = FR._upload(FR.pack_crops(p, bad), cuda)
    dev_frames = [torch.from_numpy(f).to(cuda) for f in frames]
    o32 = torch.full((3, side, side, 3), float('nan'), dtype=torch.float32, device=cuda)
    o8 = torch.full((3, side, side, 3), 77, dtype=torch.uint8, device=cuda)
    FR._launch_warp(dev_frames, recs, 3, side, o32, cuda)
    FR._launch_warp(dev_frames, recs, 3, side, o8, cuda)
    _assert_bytes_are_the_float_crops(o32, o8, 'frames_u8_to_u8')
    assert torch.equal(o8[:2], u8[:2]) and (o8[2] == 0).all() and (o32[2] == 0).all()
    # the planes kernel: frame 0 as NV12, frame 1 as an RGB descriptor
    nv12 = np.random.default_rng(22).integers(0, 256, (72, 64), dtype=np.uint8)
    table = [FR._planar(0, torch.from_numpy(nv12).to(cuda), 'nv12', 'bt601'), FR._planar(1, dev_frames[1], 'rgb', 'bt601')]
    q32 = torch.full_like(o32, float('nan'))
    q8 = torch.full_like(o8, 77)
    FR._launch_warp(table, recs, 3, side, q32, cuda)
    FR._launch_warp(table, recs, 3, side, q8, cuda)
    _assert_bytes_are_the_float_crops(q32, q8, 'planes_to_u8')
    assert torch.equal(q8[1], o8[1]) and not torch.equal(q8[0], o8[0]) and (q8[2] == 0).all()
    with pytest.raises(ValueError, match='crop_dtype'):
        warp_frames(frames, p, fi, side, device=cuda, out=o32, crop_dtype='uint8')


# ---- the chain ------------------------------------------------------------------------------------------------------

def _chain_scene():
    rng = np.random.default_rng(31)
    frames = [rng.integers(0, 256, (120, 160, 3), dtype=np.uint8), rng.integers(0, 256, (96, 128, 3), dtype=np.uint8)]
    cams = [Camera(np.array([[150., 0, 80], [0, 150., 60], [0, 0, 1]])),
            Camera(np.array([[110., 0, 64], [0, 110., 48], [0, 0, 1]]), np.array([-0.15, 0.04, 0.001, -0.001, 0.0], np.float32))]
    boxes = np.array([[20., 10., 60., 90.], [90., 30., 50., 70.], [10., 5., 70., 80.], [100., 40., 60., 80.]])
    fi = np.array([0, 0, 1, 1])
    return frames, cams, boxes, fi


@pytest.mark.parametrize('precision', ['f16', 'f64'])
def test_chain_uint8_crops_give_the_bits_of_float32_crops(cuda, toy, precision):
    """estimate_pose_in_frames and locate_poses_in_frames (bone lengths): host boxes, CUDA boxes, views=3, with one distorted
    camera among the two; nv12 frames through the planes kernel once."""
    spec, _, path = toy
    frames, cams, boxes, fi = _chain_scene()
    bones = np.random.default_rng(7).uniform(200, 450, len(spec.skeleton.head_edges))
    dboxes, dfi = torch.from_numpy(boxes).to(cuda), torch.from_numpy(fi).to(cuda)
    cases = (('host boxes', boxes, fi, None), ('cuda boxes', dboxes, dfi, None), ('views=3', boxes, fi, 3),
             ('cuda boxes, views=3', dboxes, dfi, 3))
    for what, b, f, views in cases if precision == 'f16' else cases[::3]:      # f64: the first and the last
        kw = dict(cameras=cams, frame_index=f, precision=precision, views=views)
        want = estimate_pose_in_frames(frames, b, path, **kw)[0]
        got = estimate_pose_in_frames(frames, b, path, crop_dtype='uint8', **kw)[0]
        assert torch.isfinite(want).all() and torch.equal(_bits(got), _bits(want)), (precision, what)
        lw, sw = locate_poses_in_frames(frames, b, path, bone_lengths=bones, return_spread=True, **kw)
        lg, sg = locate_poses_in_frames(frames, b, path, bone_lengths=bones, return_spread=True, crop_dtype='uint8', **kw)
        for name, x, y in (('poses', lg.poses, lw.poses), ('keypoints2d', lg.keypoints2d, lw.keypoints2d),
                           ('z_offset', lg.z_offset, lw.z_offset), ('spread', sg, sw)):
            assert torch.equal(_bits(x), _bits(y)), (precision, what, name)
        assert torch.isfinite(lw.poses).all()
    nv12 = [np.random.default_rng(40 + k).integers(0, 256, (h * 3 // 2, w), dtype=np.uint8) for k, (h, w) in enumerate(((120, 160), (96, 128)))]
    kw = dict(cameras=cams, frame_index=fi, precision=precision, pixel_format='nv12')
    want = estimate_pose_in_frames(nv12, boxes, path, **kw)[0]
    assert torch.equal(_bits(estimate_pose_in_frames(nv12, boxes, path, crop_dtype='uint8', **kw)[0]), _bits(want))
