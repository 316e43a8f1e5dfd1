"""NumPy restatement of the YUV 4:2:0 -> RGB rule of metro_warp_crops_frames_planes (include/metro_hip.h): OpenCV's integer
cvtColor(COLOR_YUV2RGB_NV12 / _I420), its scalar yuv42xxp2RGB8 path, for the BT.601 (OpenCV's) and BT.709 limited-range
matrices, and the plane slicing of the one-array layouts.  Test infrastructure: the product never imports it."""
import numpy as np

# the three-decimal limited-range coefficients CY, CVR, CVG, CUG, CUB and their 20-bit fixed-point constants
COEFFICIENTS = {'bt601': (1.164, 1.596, -0.813, -0.391, 2.018), 'bt709': (1.164, 1.793, -0.533, -0.213, 2.112)}
CONSTANTS = {'bt601': (1220542, 1673527, -852492, -409993, 2116026), 'bt709': (1220542, 1880097, -558891, -223347, 2214593)}


def yuv420_to_rgb(y, u, v, matrix='bt601'):
    """Y [H, W], U, V [H/2, W/2] uint8 -> RGB uint8 [H, W, 3]: chroma of the 2x2 block, no interpolation."""
    cy, cvr, cvg, cug, cub = CONSTANTS[matrix]
    h, w = y.shape
    up = np.repeat(np.repeat(np.asarray(u, np.int64), 2, 0), 2, 1)[:h, :w] - 128
    vp = np.repeat(np.repeat(np.asarray(v, np.int64), 2, 0), 2, 1)[:h, :w] - 128
    yy = np.maximum(0, np.asarray(y, np.int64) - 16) * cy + (1 << 19)
    r = (yy + cvr * vp) >> 20                       # NumPy's >> on signed integers is the arithmetic (floor) shift
    g = (yy + cvg * vp + cug * up) >> 20
    b = (yy + cub * up) >> 20
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def nv12_planes(frame):
    """uint8 [H*3/2, W] (Y rows, then interleaved UV rows) -> (Y [H, W], U [H/2, W/2], V [H/2, W/2])."""
    h = frame.shape[0] * 2 // 3
    uv = frame[h:].reshape(h // 2, -1, 2)
    return frame[:h], uv[..., 0], uv[..., 1]


def i420_planes(frame):
    """contiguous uint8 [H*3/2, W] (Y, then U and V at W/2 bytes per row) -> (Y, U, V)."""
    h, w = frame.shape[0] * 2 // 3, frame.shape[1]
    flat, q = np.ascontiguousarray(frame).reshape(-1), h * w // 4
    return frame[:h], flat[h * w:h * w + q].reshape(h // 2, w // 2), flat[h * w + q:].reshape(h // 2, w // 2)


def nv12_frame(y, u, v):
    """The one-array NV12 layout of the planes."""
    return np.concatenate([y, np.stack([u, v], -1).reshape(u.shape[0], -1)])


def i420_frame(y, u, v):
    """The one-array I420 layout of the planes."""
    h, w = y.shape
    return np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)]).reshape(h * 3 // 2, w)


def to_rgb(frame, pixel_format, matrix='bt601'):
    """A one-array frame in pixel_format -> the RGB uint8 [H, W, 3] frame it stands for."""
    if pixel_format == 'rgb':
        return frame
    if pixel_format == 'bgr':
        return np.ascontiguousarray(frame[..., ::-1])
    planes = nv12_planes(frame) if pixel_format == 'nv12' else i420_planes(frame)
    return yuv420_to_rgb(*planes, matrix)


def random_frame(h, w, pixel_format, matrix='bt601', seed=0):
    """-> (a random one-array frame in pixel_format, the RGB uint8 [H, W, 3] frame it stands for).  The packed formats draw
    bytes from 1..255, so a pixel whose three channels are 0 is a border pixel of the warp, never a frame pixel."""
    if pixel_format in ('rgb', 'bgr'):
        src = np.random.default_rng(seed).integers(1, 256, (h, w, 3), dtype=np.uint8)
    else:
        src = (nv12_frame if pixel_format == 'nv12' else i420_frame)(*random_planes(h, w, seed))
    return src, to_rgb(src, pixel_format, matrix)


def random_planes(h, w, seed):
    """Random Y [H, W], U, V [H/2, W/2] planes over the whole byte range (every clamp of the rule is reached)."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8),
            rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8))
