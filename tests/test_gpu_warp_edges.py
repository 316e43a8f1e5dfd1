"""The three crop-warp kernels (metro_warp_crop_u8, metro_warp_crops_frames_u8, metro_warp_crops_frames_planes) on the MI355X
against the NumPy restatement of cv2.remap, to the byte, at the edges of their contract: crop sides whose square is no
multiple of 64 (a wave straddles two crop records, frames, modes and pixel formats), more crops than the capped grid covers
in one pass, every 1/32-pixel fraction pair on frames of 1 to 6 pixels, frames 32766 and 32767 pixels wide with coordinates
at and beyond the short and the int range, frames laid out inside allocations of 0xFF bytes, frame indices outside the
table, and degenerate distorted-mode records.  The scenes and their references (tests.oracle_frames.crop_frames_u8 on the
RGB image each frame stands for, never another kernel) come from tests/test_warp_edges.py, which also proves on the CPU
that each one is non-vacuous; every comparison here is np.array_equal on the fp32 crops.

Wall times of the first run (MI355X, 2026-10-17): the 36 tests in 3.5 s, references included; the slowest are the 33 crops of
256^2 at 0.20 s per entry, side 320 at 0.17 s and the fraction sweep over all formats at 0.14 s; the others 0.02 s or less."""
import ctypes as C

import numpy as np
import pytest
import torch

from metro_pose3d_amd import _lib
from metro_pose3d_amd import frames as FR
from metro_pose3d_amd.frames import warp_frames
from metro_pose3d_amd.preprocess import warp_crops
from tests import oracle_yuv as OY
from tests import test_warp_edges as WE

pytestmark = pytest.mark.gpu

SINGLE, FRAMES, PLANES = 'warp_crop_u8', 'warp_crops_frames_u8', 'warp_crops_frames_planes'
ENTRIES = (SINGLE, FRAMES, PLANES)
MULTI_FRAME_ENTRIES = (FRAMES, PLANES)


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _assert_bytes(got, ref, what, crops=None):
    """np.array_equal on the crops; on failure the count of differing values and the largest difference in LSB."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float32
    for i in range(len(ref)) if crops is None else crops:
        if not np.array_equal(got[i], ref[i]):
            diff = got[i] != ref[i]
            raise AssertionError(f'{what}: crop {i}: {int(diff.sum())} of {diff.size} values differ, '
                                 f'max {np.abs(got[i] - ref[i]).max() * 255:.2f} LSB')


def _warp_crop_u8_pitched(frame, homs, side):
    """metro_warp_crop_u8 on a device frame [H, W, 3] with any row stride (preprocess.warp_crops packs its frame)."""
    assert frame.stride(2) == 1 and frame.stride(1) == 3
    hom = _dev(np.asarray(homs, np.float32).reshape(-1, 9), frame.device)
    out = torch.empty((len(hom), side, side, 3), dtype=torch.float32, device=frame.device)
    stream = torch.cuda.current_stream(frame.device).cuda_stream
    _lib.check(_lib.load().metro_warp_crop_u8(C.c_void_p(frame.data_ptr()), frame.shape[0], frame.shape[1], frame.stride(0),
                                              C.c_void_p(hom.data_ptr()), len(hom), side, C.c_void_p(out.data_ptr()),
                                              C.c_void_p(stream)), 'metro_warp_crop_u8')
    return out


def _run_single(cuda, scene, frames=None):
    """metro_warp_crop_u8: one launch per frame over that frame's homography-mode crops.  frames: device frames to use in
    place of the scene's (pitched ones go to the C entry directly).  -> (crops, the indices of the crops that were run)."""
    got = np.full(scene.ref.shape, np.nan, np.float32)
    ran = []
    for k, f in enumerate(scene.frames):
        sel = np.flatnonzero((scene.frame_index == k) & (scene.params.mode == 0))
        if not len(sel):
            continue
        if frames is None:
            out = warp_crops(_dev(f.rgb, cuda), scene.params.homography[sel], scene.side)
        else:
            out = _warp_crop_u8_pitched(frames[k], scene.params.homography[sel], scene.side)
        got[sel] = out.cpu().numpy()
        ran += sel.tolist()
    return got, sorted(ran)


def _run_frames(cuda, scene, frames=None, direct=False):
    """metro_warp_crops_frames_u8 on the RGB image of every frame of the table, through frames.warp_frames; direct: the
    launch warp_frames makes, without its host check of the frame indices."""
    frames = [_dev(f.rgb, cuda) for f in scene.frames] if frames is None else frames
    if not direct:
        return warp_frames(frames, scene.params, scene.frame_index, scene.side, device=cuda)
    n = len(scene.frame_index)
    out = torch.empty((n, scene.side, scene.side, 3), dtype=torch.float32, device=cuda)
    FR._launch_warp(frames, FR._upload(FR.pack_crops(scene.params, scene.frame_index), cuda), n, scene.side, out, cuda)
    return out


def _run_planes(cuda, scene, frames=None):
    """metro_warp_crops_frames_planes: one launch over the table in its own pixel formats ('rgb' frames as METRO_PIX_RGB
    descriptors).  frames: per frame a device tensor or tuple of plane views to use in place of the scene's arrays."""
    srcs = [_dev(f.src, cuda) for f in scene.frames] if frames is None else frames
    table = [FR._planar(k, src, f.pixel_format, f.color_matrix) for k, (src, f) in enumerate(zip(srcs, scene.frames))]
    n = len(scene.frame_index)
    out = torch.empty((n, scene.side, scene.side, 3), dtype=torch.float32, device=cuda)
    FR._launch_warp(table, FR._upload(FR.pack_crops(scene.params, scene.frame_index), cuda), n, scene.side, out, cuda)
    return out


def _compare(cuda, entry, scene, what, **kw):
    """Runs the scene on one entry and compares every crop the entry computes with the reference.  -> the crops."""
    if entry == SINGLE:
        got, ran = _run_single(cuda, scene, **kw)
        assert len(ran) >= 2
        _assert_bytes(got, scene.ref, f'{what} {entry}', ran)
        return got
    got = (_run_frames if entry == FRAMES else _run_planes)(cuda, scene, **kw).cpu().numpy()
    _assert_bytes(got, scene.ref, f'{what} {entry}')
    return got


# ---- 1. sides where a wave straddles two crops ----------------------------------------------------------------------------

@pytest.mark.parametrize('side', sorted(WE.STRADDLE_CROPS))
@pytest.mark.parametrize('entry', ENTRIES)
def test_sides_off_the_wave_grid(cuda, entry, side):
    """side^2 is no multiple of 64, so waves cover the end of one crop and the start of the next, whose records differ in
    frame (size and row stride), mode, matrices and, for the planes entry, pixel format and colour matrix."""
    scene = WE.straddle_scene(side, entry == PLANES)
    WE.check_non_vacuous(scene)
    WE.check_border_and_content(scene, per_crop=side >= 20)
    _compare(cuda, entry, scene, f'side {side}')


@pytest.mark.parametrize('entry', ENTRIES)
def test_side_320(cuda, entry):
    scene = WE.side320_scene(entry == PLANES)
    WE.check_non_vacuous(scene)
    WE.check_border_and_content(scene)
    _compare(cuda, entry, scene, 'side 320')


# ---- 2. the grid-stride loop's second pass --------------------------------------------------------------------------------

@pytest.mark.parametrize('entry', ENTRIES)
def test_more_crops_than_one_pass_of_the_grid(cuda, entry):
    """33 crops of 256^2: 64 K pixels more than the 8192 blocks of 256 threads cover, so the first 65 536 threads take a
    second trip through the loop; the last crop is written by that trip alone."""
    scene = WE.grid_stride_scene(entry == SINGLE)
    WE.check_non_vacuous(scene)
    WE.check_border_and_content(scene)
    assert scene.ref[-1].any()
    got = _compare(cuda, entry, scene, '33 crops')
    assert got[-1].any() and np.array_equal(got[-1], scene.ref[-1])


# ---- 3. every fraction pair on the smallest frames ------------------------------------------------------------------------

@pytest.mark.parametrize('entry', ENTRIES)
def test_fraction_sweep_over_tiny_frames(cuda, entry):
    """A 1/32-per-pixel zoom across frames of 1 x 1 to 2 x 6 pixels (4:2:0 ones of a single chroma sample among them): all
    1024 fraction pairs, against every edge of every frame."""
    scene = WE.sweep_scene(entry == PLANES)
    WE.check_non_vacuous(scene)
    assert {f.rgb.shape[:2] for f in scene.frames} >= {(2, 3), (1, 1), (1, 7), (5, 1), (2, 2)}
    if entry == PLANES:
        yuv = {(f.pixel_format, f.color_matrix, f.rgb.shape[:2]) for f in scene.frames if f.pixel_format in ('nv12', 'i420')}
        assert len(yuv) == 12
    _compare(cuda, entry, scene, 'fraction sweep')


# ---- 4. the short range on the widest frames ------------------------------------------------------------------------------

@pytest.mark.parametrize('entry,pixel_format', [(SINGLE, 'rgb'), (FRAMES, 'rgb'), (PLANES, 'rgb'), (PLANES, 'nv12'), (PLANES, 'i420')])
def test_the_short_range_on_the_widest_frames(cuda, entry, pixel_format):
    """Frames 32767 (RGB) and 32766 (4:2:0) pixels wide: the last column is sampled, a coordinate saturated to the short
    range, beyond the int range, infinite or NaN is not."""
    scene = WE.wide_scene(pixel_format)
    WE.check_wide_scene(scene)
    got = _compare(cuda, entry, scene, f'wide {pixel_format}')
    for i in scene.zero_crops:
        if entry != SINGLE or scene.params.mode[i] == 0:                  # metro_warp_crop_u8 has the homography mode only
            assert (got[i] == 0).all(), i


# ---- 5. frames inside allocations of 0xFF ---------------------------------------------------------------------------------

def _poisoned(cuda, rows, row_bytes, guard=3, pad=13):
    """A [rows, row_bytes] view into an allocation of 0xFF bytes: `guard` rows above and below, `pad` bytes to the right."""
    alloc = torch.full((rows + 2 * guard, row_bytes + pad), 0xFF, dtype=torch.uint8, device=cuda)
    return alloc[guard:guard + rows, :row_bytes]


def _poisoned_layout(cuda, f):
    """Frame f laid out in 0xFF: packed rows with a pitch of 3 w + 13; NV12 as Y and UV views of one pitched surface with
    guard rows between the planes; I420 as three planes, the chroma planes with a pitch of their own."""
    h, w = f.rgb.shape[:2]
    if f.pixel_format in ('rgb', 'bgr'):
        view = _poisoned(cuda, h, 3 * w).unflatten(1, (w, 3))
        view.copy_(_dev(f.src, cuda))
        assert view.stride() == (3 * w + 13, 3, 1)
        return view
    if f.pixel_format == 'nv12':
        surface = _poisoned(cuda, h + 3 + h // 2, w, pad=10)
        y, uv = surface[:h], surface[h + 3:]
        y.copy_(_dev(f.src[:h], cuda))
        uv.copy_(_dev(f.src[h:], cuda))
        return y, uv
    planes = OY.i420_planes(f.src)
    views = (_poisoned(cuda, h, w), _poisoned(cuda, h // 2, w // 2, pad=9), _poisoned(cuda, h // 2, w // 2, pad=9))
    for v, p in zip(views, planes):
        v.copy_(_dev(p, cuda))
    return views


@pytest.mark.parametrize('entry', ENTRIES)
def test_padding_is_never_read(cuda, entry):
    """Every frame sits in an allocation whose other bytes are 0xFF (rows above and below, the pitch to its right, between
    the planes), and every crop reaches beyond all four edges of its frame: a tap taken one pixel or one row outside the
    frame reads 255 where the border value is 0.  Side 100 also straddles waves."""
    scene = WE.padding_scene()
    WE.check_non_vacuous(scene)
    WE.check_border_and_content(scene)
    if entry == PLANES:
        frames = [_poisoned_layout(cuda, f) for f in scene.frames]
    else:
        frames = [_poisoned_layout(cuda, WE.Frame('rgb', 'bt601', f.rgb, f.rgb)) for f in scene.frames]
    _compare(cuda, entry, scene, 'poisoned padding', frames=frames)


# ---- 6. a frame index outside the table, on the device --------------------------------------------------------------------

@pytest.mark.parametrize('entry', MULTI_FRAME_ENTRIES)
def test_frame_index_outside_the_table(cuda, entry):
    """Records whose frame is -1, n_frames, 2^30 or INT_MIN come out as zeros and their neighbours in the same wave as the
    oracle's crops (the host check of frames.warp_frames is bypassed: device boxes rely on the kernel's); a mode other than
    0 or 1 takes the homography chain."""
    scene = WE.bad_frame_scene(entry == PLANES)
    WE.check_non_vacuous(scene)
    assert all(not 0 <= scene.frame_index[i] < len(scene.frames) for i in WE.BAD_FRAMES)
    with pytest.raises(ValueError, match='frame_index'):
        warp_frames([_dev(f.rgb, cuda) for f in scene.frames], scene.params, scene.frame_index, scene.side, device=cuda)
    got = _compare(cuda, entry, scene, 'bad frame index', **({'direct': True} if entry == FRAMES else {}))
    for i in WE.BAD_FRAMES:
        assert (got[i] == 0).all(), i


# ---- 7. degenerate distorted-mode records ---------------------------------------------------------------------------------

@pytest.mark.parametrize('entry', MULTI_FRAME_ENTRIES)
def test_distorted_mode_degeneracies(cuda, entry):
    """Rays with z exactly 0, a denormal z (inf rays, NaN polynomial), z < 0, NaN and inf matrix entries, coefficients that
    push u, v beyond the short and the int range: the reference decides the bytes; behind the camera and at NaN / inf
    coordinates they are 0."""
    scene = WE.degenerate_scene(entry == PLANES)
    dead = WE.check_degenerate_scene(scene)
    got = _compare(cuda, entry, scene, 'degenerate records')
    assert dead.any() and not got[dead].any()
    for i in scene.zero_crops:
        assert not got[i].any(), i
