"""The crop warp's reference at the shapes of tests/test_gpu_warp_edges.py, without a GPU: NumPy's float32 matmul against the
explicit coordinate chains the kernels document at every crop side used there, known answers of the restated cv2.remap on
a hand-written 2 x 3 frame under a 1/32-per-pixel zoom (every fraction pair, the zero border on all sides, floor semantics
of negative fixed-point coordinates), and the scenes of the GPU comparisons with the check that each one is non-vacuous.

A scene is a frame table (each frame in its pixel format, with the RGB image it stands for) and MetroCropWarp parameters;
its reference is tests.oracle_frames.crop_frames_u8 on those RGB images, computed once per process and read-only."""
import functools
from typing import NamedTuple

import numpy as np
import pytest

from metro_pose3d_amd.frames import CropParams
from oracle.preprocess import crop_coordinates, cv_round_x86, reproject_image_u8
from tests import oracle_frames as OP
from tests import oracle_yuv as OY

# every crop side of tests/test_gpu_warp_edges.py: 1, 3, 20, 33, 100 (side^2 is no multiple of 64: waves straddle crops), 64
# (the wide frames), 160 (the fraction sweep), 256 (the grid-stride pass), 320
SIDES = (1, 3, 20, 33, 64, 100, 160, 256, 320)
F32 = np.float32


def _fma32(a, b, c):
    """fma(a, b, c) on float32 arrays: the product of two float32 is exact in float64."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


# ---- A. the reference's coordinates are the chains the kernels evaluate ---------------------------------------------------

@pytest.mark.parametrize('side', SIDES)
def test_homography_coordinates_are_the_fma_chain_at_every_side(side):
    """crop_coordinates (NumPy's float32 matmul of a 3 x side^2 product, whose BLAS path may depend on side^2) against
    fma(h2, 1, fma(h1, y, rn(h0 x))) and the IEEE divide, bit for bit, six homographies per side."""
    y, x = np.mgrid[:side, :side].astype(F32)
    for seed in range(6):
        rng = np.random.default_rng(1000 * side + seed)
        hom = (rng.standard_normal((3, 3)) * np.array([[1, 0.1, 300], [0.1, 1, 200], [1e-4, 1e-4, 1]])).astype(F32)
        mapx, mapy = crop_coordinates(hom, side)
        rows = [_fma32(hom[r, 2], 1, _fma32(hom[r, 1], y, hom[r, 0] * x)) for r in range(3)]
        assert rows[0].dtype == F32 and (hom[0, 0] * x).dtype == F32
        assert np.array_equal(mapx, rows[0] / rows[2]) and np.array_equal(mapy, rows[1] / rows[2]), (side, seed)


@pytest.mark.parametrize('side', SIDES)
def test_projection_coordinates_are_the_fma_chain_at_every_side(side):
    """project_points ends in `projected @ K[:2, :2].T + K[:2, 2]` (reference cameralib.py:397), a [side^2, 2] x [2, 2]
    float32 matmul; tests.oracle_frames.project_points and the kernel evaluate fma(py, K01, rn(px K00)) + K02.  NumPy itself
    against that chain, bit for bit, six skewed intrinsic matrices per side (a plain rn(px K00) + rn(py K01) differs in about
    a quarter of the values).  At side 1 the product has one row and NumPy hands it to a matrix-vector routine that sums in
    the other order, fma(px, K00, rn(py K01)): a last-bit difference in about a quarter of the values.  There the explicit
    chain, which the kernel documents and tests.oracle_frames.project_points evaluates at every side, is the reference, and
    NumPy is only held to one ulp of it."""
    for seed in range(6):
        rng = np.random.default_rng(2000 * side + seed)
        pts = (rng.standard_normal((side * side, 2)) * 0.7).astype(F32)
        k = np.array([[1100 + 50 * rng.standard_normal(), 3 * rng.standard_normal(), 640 + 20 * rng.standard_normal()],
                      [2 * rng.standard_normal(), 1090 + 50 * rng.standard_normal(), 360 + 20 * rng.standard_normal()],
                      [0, 0, 1]]).astype(F32)
        got = pts @ k[:2, :2].T + k[:2, 2]
        assert got.dtype == F32
        px, py = pts[:, 0], pts[:, 1]
        u = _fma32(py, k[0, 1], px * k[0, 0]) + k[0, 2]
        v = _fma32(py, k[1, 1], px * k[1, 0]) + k[1, 2]
        want = np.stack([u, v], -1)
        if side > 1:
            assert np.array_equal(got, want), (side, seed)
        else:
            assert (np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want))).all(), seed
        # and the oracle's own statement of it, through a distortion-free project_points
        ou, ov = OP.project_points(np.concatenate([pts, np.ones((len(pts), 1), F32)], 1), k, np.zeros(5, F32))
        assert np.array_equal(ou, u) and np.array_equal(ov, v), (side, seed)


# ---- A. known answers of the oracle on the fraction sweep -----------------------------------------------------------------

SWEEP_SIDE = 160
SWEEP_FRAME = np.array([[[200, 1, 90], [100, 2, 80], [50, 3, 70]],
                        [[10, 4, 60], [250, 5, 40], [255, 6, 30]]], np.uint8)            # 2 x 3 (h x w), bytes chosen by hand


def sweep_homography(x0=-1.5, y0=-1.5):
    """A zoom of 1/32 source pixel per output pixel from (x0, y0): output pixel (x, y) samples (x0 + x / 32, y0 + y / 32)."""
    return np.array([[1 / 32, 0, x0], [0, 1 / 32, y0], [0, 0, 1]], F32)


def test_the_fraction_sweep_reaches_every_fraction_pair_and_the_zero_border():
    h, w = SWEEP_FRAME.shape[:2]
    mapx, mapy = crop_coordinates(sweep_homography(), SWEEP_SIDE)
    y, x = np.mgrid[:SWEEP_SIDE, :SWEEP_SIDE]
    assert np.array_equal(mapx, x / 32 - 1.5) and np.array_equal(mapy, y / 32 - 1.5)        # exact in float32
    sx, sy = cv_round_x86(mapx * F32(32)), cv_round_x86(mapy * F32(32))
    assert np.array_equal(sx, x - 48) and np.array_equal(sy, y - 48)
    assert len({(int(a), int(b)) for a, b in zip((sx & 31).ravel(), (sy & 31).ravel())}) == 32 * 32
    # sx < 0: `>> 5` and `& 31` are floor and its remainder (-48 = -2 * 32 + 16, -1 = -1 * 32 + 31), not truncation
    assert (sx[0, 0] >> 5, sx[0, 0] & 31) == (-2, 16) and (sx[0, 47] >> 5, sx[0, 47] & 31) == (-1, 31)
    assert np.array_equal(sx >> 5, np.floor(mapx.astype(np.float64))) and np.array_equal(sx & 31, sx - 32 * (sx >> 5))
    out = reproject_image_u8(SWEEP_FRAME, sweep_homography(), SWEEP_SIDE).astype(np.int64)
    img = SWEEP_FRAME.astype(np.int64)
    # bytes by hand, channel 0 (a, b, c = 200, 100, 50 in row 0; 10, 250, 255 in row 1)
    assert out[48, 48, 0] == 200 and out[80, 112, 0] == 255                    # exact grid points (0, 0) and (2, 1)
    assert out[48, 47, 0] == 194                                               # u = -1/32: (200 * 31 * 1024 + 2^14) >> 15
    assert out[32, 32, 0] == 50                                                # (-0.5, -0.5): (200 * 8192 + 2^14) >> 15
    assert out[48, 128, 0] == 25                                               # u = 2.5 in (w - 1, w): (50 + 1) >> 1
    assert out[96, 48, 0] == 5                                                 # v = 1.5 in (h - 1, h): (10 + 1) >> 1
    assert out[72, 56, 0] == 96       # (0.25, 0.75): (200 * 6144 + 100 * 2048 + 10 * 18432 + 250 * 6144 + 2^14) >> 15
    # every coordinate in (-1, 0) and (w - 1, w) blends one column with the zero border: (S (32 - a) + 16) >> 5, (S a + 16) >> 5
    for col, src_col, weight in ((np.arange(17, 48), 0, np.arange(17, 48) - 16), (np.arange(113, 144), w - 1, 144 - np.arange(113, 144))):
        assert np.array_equal(out[48, col], (img[0, src_col][None] * weight[:, None] + 16) >> 5)
    for row, src_row, weight in ((np.arange(17, 48), 0, np.arange(17, 48) - 16), (np.arange(81, 112), h - 1, 112 - np.arange(81, 112))):
        assert np.array_equal(out[row, 48], (img[src_row, 0][None] * weight[:, None] + 16) >> 5)
    # at and beyond one pixel outside: the border value
    assert (out[:, :17] == 0).all() and (out[:, 144:] == 0).all() and (out[:17] == 0).all() and (out[112:] == 0).all()
    assert (out[48:81, 48:113] > 0).all()                                      # inside the frame: positive bytes only


# ---- the scenes of tests/test_gpu_warp_edges.py ---------------------------------------------------------------------------

class Frame(NamedTuple):
    pixel_format: str            # 'rgb', 'bgr', 'nv12', 'i420'
    color_matrix: str            # 'bt601', 'bt709' (the YUV formats)
    src: np.ndarray              # the one-array frame in pixel_format
    rgb: np.ndarray              # the RGB uint8 [H, W, 3] frame it stands for


class Scene(NamedTuple):
    side: int
    frames: tuple                # the frame table
    params: CropParams           # as packed into the MetroCropWarp records
    frame_index: np.ndarray      # int64 [n], as packed
    ref: np.ndarray              # float32 [n, side, side, 3], read-only
    zero_crops: tuple = ()       # crops whose purpose is an all-zero output (exempt from the non-vacuity checks)


FORMATS = (('rgb', 'bt601'), ('bgr', 'bt601'), ('nv12', 'bt601'), ('i420', 'bt709'), ('nv12', 'bt709'), ('i420', 'bt601'))


def make_frame(h, w, pixel_format='rgb', color_matrix='bt601', seed=0) -> Frame:
    src, rgb = OY.random_frame(h, w, pixel_format, color_matrix, seed)
    return Frame(pixel_format, color_matrix, src, rgb)


def _rot(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    m = {'y': [[c, 0, s], [0, 1, 0], [-s, 0, c]], 'z': [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis]
    return np.array(m)


def homography_record(h, w, side, i, cover=False):
    """A float32 homography into an h x w frame that differs with i in zoom, offset (fractional), shear and perspective;
    cover: the crop reaches beyond all four edges of the frame."""
    zoom = 1.5 if cover else (0.7, 1.0, 1.4)[i % 3]
    sx, sy = zoom * w / side, zoom * h / side
    x0 = (-0.25 if cover else -0.2 + 0.2 * (i % 4)) * w + (i % 7) / 7
    y0 = (-0.25 if cover else -0.2 + 0.25 * (i % 3)) * h + (i % 5) / 5
    shear = 0.1 * ((i % 3) - 1)
    return np.array([[sx, shear * sx, x0], [-shear * sy, sy, y0], [0.1 / side * (i % 2), 0, 1]], F32)


def distorted_record(h, w, side, i, cover=False):
    """(partial float64 [3, 3], intrinsics float32 [3, 3], distortion float32 [5]) of a lens-distorted camera over an h x w
    frame, differing with i in the virtual camera's principal point and rotation and in the original camera's skew,
    principal point and coefficients; cover: the rays reach beyond all four edges."""
    f = side / 1.2                                                     # rays span 1.2 around the principal point
    cx, cy = side * (0.5 if cover else 0.1 + 0.15 * (i % 5)), side * (0.5 if cover else 0.1 + 0.1 * (i % 4))
    rot = _rot('y', 0.06 * ((i % 5) - 2)) @ _rot('z', 0.1 * (i % 3))
    partial = rot @ np.linalg.inv(np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]]))
    g = 1.4 if cover else 1.0
    k = np.array([[g * w, 0.25 * (i % 2), w / 2 + (i % 4)], [0, g * h, h / 2 - (i % 3)], [0, 0, 1]], F32)
    dist = (np.array([-0.2, 0.08, 0.002, -0.001, 0.01]) * (0.5 + 0.25 * (i % 4))).astype(F32)
    return partial, k, dist


def empty_params(n) -> CropParams:
    return CropParams(np.zeros(n, np.int32), np.zeros((n, 3, 3), F32), np.zeros((n, 3, 3)), np.zeros((n, 3, 3), F32),
                      np.zeros((n, 5), F32), None, None)


def fill_records(frames, fi, modes, side, cover=False) -> CropParams:
    """The parameters of len(fi) crops: crop i of frame fi[i] in mode modes[i], every record different."""
    p = empty_params(len(fi))
    for i, (f, m) in enumerate(zip(fi, modes)):
        h, w = frames[f].rgb.shape[:2]
        v = i + i // len(frames)                     # the variant: a frame's crops do not share i modulo 3, 4 or 5
        p.mode[i] = m
        if m == 0:
            p.homography[i] = homography_record(h, w, side, v, cover)
        else:
            p.partial[i], p.intrinsics[i], p.distortion[i] = distorted_record(h, w, side, v, cover)
    return p


def reference(frames, p: CropParams, fi, side, mode=None) -> np.ndarray:
    ref = OP.crop_frames_u8([f.rgb for f in frames], fi, p.mode if mode is None else mode, p.homography, p.partial, p.intrinsics,
                            p.distortion, side)
    ref.setflags(write=False)
    return ref


def _scene(frames, p, fi, side, ref=None, zero_crops=()) -> Scene:
    fi = np.asarray(fi, np.int64)
    return Scene(side, tuple(frames), p, fi, reference(frames, p, fi, side) if ref is None else ref, tuple(zero_crops))


STRADDLE_SIZES = ((38, 54), (64, 48))            # two frame sizes: two row strides in every format
STRADDLE_CROPS = {1: 144, 3: 48, 20: 24, 33: 24, 100: 24}


def _alternating(n, n_frames):
    """(frame index, mode) of n crops: neighbours always differ in the frame and in every second pair in the mode; over the
    crops every frame meets both modes."""
    i = np.arange(n)
    return i % n_frames, ((i + 1) // 2 + i // max(n_frames, 4)) % 2


@functools.lru_cache(maxsize=None)
def straddle_scene(side: int, mixed_formats: bool) -> Scene:
    """Item 1 at the sides whose square is no multiple of 64.  mixed_formats False: two RGB frames of different sizes;
    True: twelve frames, every (size, format / matrix) pair, neighbours in the table differing in both."""
    if mixed_formats:
        frames = [make_frame(*STRADDLE_SIZES[k % 2], *FORMATS[(k + 3 * (k // 6)) % 6], seed=100 + k) for k in range(12)]
    else:
        frames = [make_frame(*STRADDLE_SIZES[k], seed=120 + k) for k in range(2)]
    fi, modes = _alternating(STRADDLE_CROPS[side], len(frames))
    return _scene(frames, fill_records(frames, fi, modes, side), fi, side)


@functools.lru_cache(maxsize=None)
def side320_scene(mixed_formats: bool) -> Scene:
    """Item 1 above side 256: 2 frames, 7 crops."""
    formats = (('i420', 'bt601'), ('nv12', 'bt709')) if mixed_formats else (('rgb', 'bt601'),) * 2
    frames = [make_frame(*size, *fmt, seed=130 + k) for k, (size, fmt) in enumerate(zip(((240, 320), (180, 122)), formats))]
    fi, modes = _alternating(7, 2)
    return _scene(frames, fill_records(frames, fi, modes, 320), fi, 320)


GRID_STRIDE_CROPS = 33                           # 33 * 256^2 outputs: the first count above the launchers' 8192 x 256 threads
GRID_STRIDE_SIZES = ((120, 160), (96, 128), (150, 110), (64, 200))


@functools.lru_cache(maxsize=None)
def grid_stride_scene(single_frame: bool) -> Scene:
    """Item 2: 33 crops at side 256.  single_frame False: 4 frames (RGB, BGR, NV12, I420), both modes mixed; True: every
    crop a homography of frame 0 (metro_warp_crop_u8)."""
    frames = [make_frame(*GRID_STRIDE_SIZES[k], *FORMATS[k], seed=140 + k) for k in range(1 if single_frame else 4)]
    if single_frame:
        fi, modes = np.zeros(GRID_STRIDE_CROPS, np.int64), np.zeros(GRID_STRIDE_CROPS, np.int64)
    else:
        fi, modes = _alternating(GRID_STRIDE_CROPS, 4)
    return _scene(frames, fill_records(frames, fi, modes, 256), fi, 256)


TINY_RGB_SIZES = ((1, 1), (1, 7), (5, 1), (2, 2))
TINY_YUV_SIZES = ((2, 2), (2, 6), (4, 2))


@functools.lru_cache(maxsize=None)
def sweep_scene(mixed_formats: bool) -> Scene:
    """Item 3: the 1/32-per-pixel zoom at side 160 over the hand-written 2 x 3 frame and frames of 1 x 1, 1 x 7, 5 x 1 and 2 x 2
    (mixed_formats: those as RGB and BGR, and 4:2:0 frames of 2 x 2, 2 x 6 and 4 x 2 in NV12 and I420 with both matrices).
    Every frame is swept from (-1.5, -1.5) and from (w - 3.5, h - 3.5), so all four edges are crossed at every fraction, in
    the homography mode and, with the same coordinates (identity intrinsics, no distortion), in the distorted mode."""
    frames = [Frame('rgb', 'bt601', SWEEP_FRAME, SWEEP_FRAME)] + [make_frame(h, w, seed=150 + k) for k, (h, w) in enumerate(TINY_RGB_SIZES)]
    if mixed_formats:
        frames[1::2] = [Frame('bgr', 'bt601', np.ascontiguousarray(f.rgb[..., ::-1]), f.rgb) for f in frames[1::2]]
        frames += [make_frame(h, w, fmt, matrix, seed=160 + k) for k, (h, w) in enumerate(TINY_YUV_SIZES)
                   for fmt in ('nv12', 'i420') for matrix in ('bt601', 'bt709')]
    fi = np.repeat(np.arange(len(frames)), 4)
    p = empty_params(len(fi))
    for i, f in enumerate(fi):
        h, w = frames[f].rgb.shape[:2]
        hom = sweep_homography() if i % 4 < 2 else sweep_homography(w - 3.5, h - 3.5)
        p.mode[i] = i % 2
        p.homography[i] = hom
        p.partial[i], p.intrinsics[i] = hom.astype(np.float64), np.eye(3, dtype=F32)
    return _scene(frames, p, fi, SWEEP_SIDE)


WIDE_SIDE = 64
WIDE_X0 = 32740                                  # the first u of the in-frame crops


def wide_homographies():
    """Item 4: a translation in u, u = x + t (or a quotient whose divisor crosses 0); v is the constant 0 or 0.5 over the
    crop (row 1 of the matrix is (0, 0, v)), so all 64 rows of a crop lie in the 2-row frame and the scene is non-vacuous.
    The first four are partly inside a frame 32766 or 32767 wide (u through 32765.0 ... 32768.0 in half steps); the others
    saturate."""
    def shift(t, v):
        return [[1, 0, t], [0, 0, v], [0, 0, 1]]
    homs = [shift(WIDE_X0, 0), shift(WIDE_X0 + 0.5, 0.5), shift(WIDE_X0 + 0.5, 0), shift(WIDE_X0, 0.5),
            shift(40000 - 10, 0), shift(-40000 - 10, 0.5),                                   # beyond the short range
            shift(2.0 ** 31 / 32 - 32, 0), shift(-2.0 ** 31 / 32 - 32, 0.5),                 # 32 u reaches +-2^31
            [[1, 0, WIDE_X0], [0, 0, 0], [-1 / 32, 0, 1]],                                   # cw = 0 at x = 32: +inf, v = 0 / 0
            [[1, 0, -1e5], [0, 0, 0.5], [-1 / 32, 0, 1]],                                    # -inf
            [[1, 0, -32], [0, 0, 0.5], [-1 / 32, 0, 1]]]                                     # 0 / 0 in u
    return np.array(homs, F32)


WIDE_SATURATED = tuple(range(4, 8)) + (9, 10)    # wholly outside every frame: all zeros


@functools.lru_cache(maxsize=None)
def wide_scene(pixel_format: str) -> Scene:
    """Item 4: one 2 x 32767 RGB frame, or one 2 x 32766 NV12 / I420 frame; wide_homographies in the homography mode and, for
    the entries that have it, the same coordinates through the distorted mode."""
    w = 32767 if pixel_format == 'rgb' else 32766
    frames = [make_frame(2, w, pixel_format, 'bt601' if pixel_format == 'rgb' else 'bt709', seed=170)]
    homs = wide_homographies()
    n = len(homs)
    p = empty_params(2 * n)
    p.homography[:n] = p.homography[n:] = homs
    p.mode[n:] = 1
    p.partial[:], p.intrinsics[:] = p.homography.astype(np.float64), np.eye(3, dtype=F32)
    zero = WIDE_SATURATED + tuple(n + i for i in WIDE_SATURATED)
    return _scene(frames, p, np.zeros(2 * n, np.int64), WIDE_SIDE, zero_crops=zero)


PADDING_SIDE = 100
PADDING_SIZE = (38, 54)


@functools.lru_cache(maxsize=None)
def padding_scene() -> Scene:
    """Item 5: four frames of one size (RGB, BGR, NV12, I420), four crops each, both modes, every crop beyond all four
    edges of its frame.  The GPU test lays each frame out inside a larger allocation of 0xFF bytes."""
    frames = [make_frame(*PADDING_SIZE, *FORMATS[k], seed=180 + k) for k in range(4)]
    fi, modes = _alternating(16, 4)
    return _scene(frames, fill_records(frames, fi, modes, PADDING_SIDE, cover=True), fi, PADDING_SIDE)


BAD_FRAME_SIDE = 20
BAD_FRAMES = {1: -1, 4: None, 7: 2 ** 30, 10: -2 ** 31, 13: None}      # crop -> packed frame index (None: n_frames)
ODD_MODE_CROPS = (3, 8)                                                  # packed with mode 7: the homography chain


@functools.lru_cache(maxsize=None)
def bad_frame_scene(mixed_formats: bool) -> Scene:
    """Item 6: the side-20 scene of item 1 whose records BAD_FRAMES name a frame outside the table (all zeros) and whose
    ODD_MODE_CROPS carry mode 7 (the kernel's `else`: the homography chain)."""
    base = straddle_scene(BAD_FRAME_SIDE, mixed_formats)
    p = CropParams(*(None if a is None else a.copy() for a in base.params))
    fi = base.frame_index.copy()
    ref = base.ref.copy()
    oracle_mode = p.mode.copy()
    for i in ODD_MODE_CROPS:
        h, w = base.frames[fi[i]].rgb.shape[:2]
        p.homography[i] = homography_record(h, w, BAD_FRAME_SIDE, i)
        p.mode[i], oracle_mode[i] = 7, 0
    sel = np.array(ODD_MODE_CROPS)
    sub = CropParams(*(None if a is None else a[sel] for a in p))
    ref[sel] = reference(base.frames, sub, fi[sel], BAD_FRAME_SIDE, mode=oracle_mode[sel])
    for i, bad in BAD_FRAMES.items():
        fi[i] = len(base.frames) if bad is None else bad
        ref[i] = 0
    ref.setflags(write=False)
    return _scene(base.frames, p, fi, BAD_FRAME_SIDE, ref=ref, zero_crops=tuple(BAD_FRAMES))


DEGENERATE_SIDE = 33
DEGENERATE_ALL_ZERO = (1, 3, 4, 5, 6)


@functools.lru_cache(maxsize=None)
def degenerate_scene(mixed_formats: bool) -> Scene:
    """Item 7: distorted-mode records written by hand, side 33, over the frames of item 1.
      0   ray z = (x - y) / 16: exactly 0 on the diagonal, negative below it, positive above
      1   ray z = (x - y) 2^-140: 0 on the diagonal, negative below, a float32 denormal above (x / z overflows to inf and the
          polynomial to NaN)
      2   ray z = 1e-30: finite rays of 1e29 whose r^2 overflows, except the centre pixel's ray (0, 0, 1e-30)
      3-6 a NaN in the partial homography's row 0, row 1, row 2, and an inf in row 0
      7   k1 = 1e5: u, v leave the short range a few pixels from the centre
      8   k1 = 1e12: u, v leave the int range (32 u >= 2^31)
      9   k3 = 1e30 with rays of up to 3.5e7: r^6 or its product with k3 overflows everywhere but at the centre pixel
      10+ the ordinary records of their frames"""
    frames = straddle_scene(DEGENERATE_SIDE, mixed_formats).frames
    n = 14
    fi = np.arange(n) % len(frames)
    p = fill_records(frames, fi, np.ones(n, np.int64), DEGENERATE_SIDE, cover=True)
    centred = np.array([[1 / 27, 0, -16 / 27], [0, 1 / 27, -16 / 27], [0, 0, 1]])       # ray (0, 0, 1) at pixel (16, 16)
    p.partial[0] = centred
    p.partial[0, 2] = [1 / 16, -1 / 16, 0]
    p.partial[1] = centred
    p.partial[1, 2] = [2.0 ** -140, -2.0 ** -140, 0]
    p.partial[2] = centred
    p.partial[2, 2] = [0, 0, 1e-30]
    for i, at in ((3, (0, 0)), (4, (1, 1)), (5, (2, 2)), (6, (0, 2))):
        p.partial[i][at] = np.inf if i == 6 else np.nan
    p.partial[7] = p.partial[8] = centred
    p.distortion[7], p.distortion[8] = [1e5, 0, 0, 0, 0], [1e12, 0, 0, 0, 0]
    p.partial[9] = centred * np.array([[6e7], [6e7], [1]])
    p.distortion[9] = [0, 0, 0, 0, 1e30]
    return _scene(frames, p, fi, DEGENERATE_SIDE, zero_crops=DEGENERATE_ALL_ZERO)


# ---- every scene is non-vacuous -------------------------------------------------------------------------------------------

def check_non_vacuous(scene: Scene, min_fraction=0.05):
    """On the reference alone: at least 5 % of the scene's values are nonzero, and the crops named all-zero are."""
    ref = scene.ref
    assert ref.shape == (len(scene.frame_index), scene.side, scene.side, 3) and ref.dtype == F32
    assert np.count_nonzero(ref) >= min_fraction * ref.size, np.count_nonzero(ref) / ref.size
    for i in scene.zero_crops:
        assert not ref[i].any(), i
    return ref


def check_border_and_content(scene: Scene, per_crop=True):
    """Items 1, 2 and 5: for every warp mode and every pixel format (with its colour matrix) in the scene, one crop holds
    both zero pixels (the border) and nonzero pixels.  per_crop False (sides 1 and 3, whose crops are 1 and 9 pixels): the
    crops of the mode and format hold both between them."""
    zero = ~scene.ref.any(axis=-1)                                       # [n, side, side]: all three channels 0
    fmt = np.array([scene.frames[f][:2] for f in scene.frame_index])
    seen = set()
    for mode in np.unique(scene.params.mode):
        for pf, cm in sorted({tuple(r) for r in fmt}):
            sel = (scene.params.mode == mode) & (fmt[:, 0] == pf) & (fmt[:, 1] == cm)
            assert sel.any(), (mode, pf, cm)
            z = zero[sel].reshape(sel.sum(), -1)
            both = (z.any(axis=1) & ~z.all(axis=1)).any() if per_crop else (z.any() and not z.all())
            assert both, (mode, pf, cm)
            seen.add((int(mode), pf, cm))
    return seen


@pytest.mark.parametrize('mixed_formats', [False, True])
@pytest.mark.parametrize('side', sorted(STRADDLE_CROPS))
def test_the_straddle_scenes_are_non_vacuous(side, mixed_formats):
    scene = straddle_scene(side, mixed_formats)
    assert (side * side) % 64 and len(scene.frame_index) * side * side > 64           # more than one wave, none aligned
    check_non_vacuous(scene)
    seen = check_border_and_content(scene, per_crop=side >= 20)
    assert len(seen) == 2 * (6 if mixed_formats else 1)
    assert (np.diff(scene.frame_index) != 0).all() and (np.diff(scene.params.mode) != 0).any()
    if mixed_formats:       # neighbouring crops differ in frame size and in pixel format (or colour matrix)
        sizes = [scene.frames[f].rgb.shape for f in scene.frame_index]
        fmts = [scene.frames[f][:2] for f in scene.frame_index]
        assert all(a != b for a, b in zip(sizes, sizes[1:])) and all(a != b for a, b in zip(fmts, fmts[1:]))


@pytest.mark.parametrize('mixed_formats', [False, True])
def test_the_other_scenes_are_non_vacuous(mixed_formats):
    scene = side320_scene(mixed_formats)
    assert len(scene.frames) == 2 and len(scene.frame_index) == 7
    check_non_vacuous(scene)
    check_border_and_content(scene)
    check_non_vacuous(sweep_scene(mixed_formats))
    scene = bad_frame_scene(mixed_formats)
    check_non_vacuous(scene)
    n_frames = len(scene.frames)
    assert sorted(set(scene.frame_index) - set(range(n_frames))) == [-2 ** 31, -1, n_frames, 2 ** 30]
    assert (scene.params.mode[list(ODD_MODE_CROPS)] == 7).all() and scene.ref[list(ODD_MODE_CROPS)].any(axis=(1, 2, 3)).all()
    valid = np.setdiff1d(np.arange(len(scene.frame_index)), list(BAD_FRAMES))
    assert scene.ref[valid].any(axis=(1, 2, 3)).all()                    # the flagged crops' neighbours are not black
    check_degenerate_scene(degenerate_scene(mixed_formats))


def check_degenerate_scene(scene: Scene):
    """On the reference alone: the records of degenerate_scene produce what its docstring says.  -> bool [n, 33, 33]: the
    pixels behind the camera or with a NaN / inf coordinate, which are the border value."""
    ref = check_non_vacuous(scene)
    p = scene.params
    all_dead = []
    rz = lambda i: np.float32(p.partial[i, 2, 0] * np.arange(33.)[None] + p.partial[i, 2, 1] * np.arange(33.)[:, None] + p.partial[i, 2, 2])
    for i in (0, 1):
        assert (np.diag(rz(i)) == 0).all() and (rz(i) < 0).any() and (rz(i) > 0).any()
    assert (rz(1)[rz(1) > 0] < np.finfo(F32).tiny).all() and 0 < rz(2)[0, 0] < 1e-29
    for i in range(len(scene.frame_index)):
        mx, my = OP.distorted_crop_coordinates(p.partial[i], p.intrinsics[i], p.distortion[i], 33)
        dead = ~(np.isfinite(mx) & np.isfinite(my))
        assert not ref[i][dead].any()                                    # behind the camera, NaN or inf: the border value
        all_dead.append(dead)
        if i in (0, 1):
            assert dead[np.tril_indices(33)].all()
        if i in (3, 4, 5, 6):
            assert dead.all(), i
        if i in (2, 9):     # everything overflows but the centre pixel's ray, which lands on the principal point
            assert dead.sum() == 33 * 33 - 1 and ref[i, 16, 16].any(), i
        if i in (7, 8):     # in the frame at the centre, beyond the short (7) and the int (8) range away from it
            assert ref[i, 16, 16].any() and np.abs(mx).max() > (2.0 ** 31 / 32 if i == 8 else 32768)
            assert (np.abs(mx).max() < 2.0 ** 31 / 32) == (i == 7)
    return np.stack(all_dead)


@pytest.mark.parametrize('single_frame', [False, True])
def test_the_grid_stride_scene_is_non_vacuous(single_frame):
    scene = grid_stride_scene(single_frame)
    n = len(scene.frame_index)
    assert (n - 1) * 256 * 256 <= 8192 * 256 < n * 256 * 256             # only the loop's second trip writes the last crop
    check_non_vacuous(scene)
    check_border_and_content(scene)
    assert scene.ref[-1].any() and not scene.ref[-1].all()
    if not single_frame:
        assert len(scene.frames) == 4 and set(scene.params.mode) == {0, 1}


@pytest.mark.parametrize('pixel_format', ['rgb', 'nv12', 'i420'])
def test_the_wide_scene_saturates_where_it_should(pixel_format):
    """Read from the reference: the last in-frame column is nonzero, the column after it and everything whose coordinate
    saturates (short range, int range, inf, NaN) is the border value."""
    check_wide_scene(wide_scene(pixel_format))


def check_wide_scene(scene: Scene):
    ref = check_non_vacuous(scene)
    pixel_format = scene.frames[0].pixel_format
    w = scene.frames[0].rgb.shape[1]
    assert w == (32767 if pixel_format == 'rgb' else 32766)
    last = w - 1 - WIDE_X0                                               # the crop column that samples frame column w - 1
    n = len(ref) // 2
    for base in (0, n):                                                  # homography mode, distorted mode
        for i in range(4):
            crop = ref[base + i]
            assert crop[:, :last + 1].any(axis=-1).all(), (base, i)      # up to the last column (or half past it): frame pixels
            assert not crop[:, last + 1:].any(), (base, i)
        assert ref[base, 0, last].tolist() == (scene.frames[0].rgb[0, w - 1] / F32(255)).tolist()
    assert ref[8, :, 0].any() and not ref[8, :, 1:].any()                # cw = 1 at x = 0 only; then the quotient runs away
    mapx, mapy = crop_coordinates(scene.params.homography[8], WIDE_SIDE)
    assert np.isposinf(mapx[:, 32]).all() and np.isnan(mapy[:, 32]).all()
    assert np.isneginf(crop_coordinates(scene.params.homography[9], WIDE_SIDE)[0][:, 32]).all()
    assert np.isnan(crop_coordinates(scene.params.homography[10], WIDE_SIDE)[0][:, 32]).all()
    us = np.concatenate([crop_coordinates(h, WIDE_SIDE)[0][0] for h in scene.params.homography[:8]])
    for u in (32765.0, 32765.5, 32766.0, 32766.5, 32767.0, 32768.0, 40000.0, -40000.0, 2.0 ** 31 / 32, -2.0 ** 31 / 32):
        assert (us == u).any(), u


def test_the_padding_scene_is_non_vacuous():
    scene = padding_scene()
    check_non_vacuous(scene)
    assert len(check_border_and_content(scene)) == 8
    zero = ~scene.ref.any(axis=-1)
    for i in range(len(zero)):      # every crop is beyond all four edges: its outline is border, its centre is not
        assert zero[i, 0].all() and zero[i, -1].all() and zero[i, :, 0].all() and zero[i, :, -1].all() and not zero[i, 50, 50]
