"""uint8 crops at the C boundary and in the Python layer, without a GPU: which stem kernel metro_stem_pool_u8in dispatches
(dry run), what it and metro_forward_u8 reject, and the argument checks that come before any device work.  The arithmetic
itself (bit equality with the float32 path) is tests/test_gpu_u8_input.py."""
import ctypes as C

import numpy as np
import pytest

from metro_pose3d_amd import ModelSpec, _lib
from metro_pose3d_amd.engine import Engine

INVALID_ARG = -1            # MetroStatus METRO_ERR_INVALID_ARG
P = C.c_void_p(4096)          # never dereferenced: dry runs and rejected calls


@pytest.fixture
def dry(lib):
    lib.metro_kernel_notes(2)
    yield lib
    lib.metro_kernel_notes(0)


def test_stem_u8in_dispatch_ids(dry):
    assert dry.metro_stem_pool_u8in(P, P, P, P, 3, 256, None) == 0, dry.metro_last_error()
    assert dry.metro_last_kernel_id() == b'stem_pool_f16<rows,u8in>'
    dry.metro_kernel_notes(2)
    assert dry.metro_stem_pool_u8in(P, P, P, P, 2, 96, None) == 0, dry.metro_last_error()
    kid = dry.metro_last_kernel_id().decode()
    assert kid.startswith('stem_pool_f16<split') and kid.endswith(',u8in>'), kid
    # the float32 twin keeps its ids
    dry.metro_kernel_notes(2)
    assert dry.metro_stem_pool_f32in(P, P, P, P, 3, 256, None) == 0
    assert dry.metro_last_kernel_id() == b'stem_pool_f16<rows,f32in>'


def test_stem_u8in_rejects_bad_arguments(dry):
    for side in (100, 0, 16):
        assert dry.metro_stem_pool_u8in(P, P, P, P, 1, side, None) == INVALID_ARG
        assert b'stem_pool_u8in' in dry.metro_last_error() and b'side' in dry.metro_last_error()
    assert dry.metro_stem_pool_u8in(None, P, P, P, 1, 256, None) == INVALID_ARG
    assert b'NULL' in dry.metro_last_error()
    assert dry.metro_stem_pool_u8in(P, P, P, None, 1, 256, None) == INVALID_ARG
    for side in (256, 96):
        for off in (1, 4, 8):
            assert dry.metro_stem_pool_u8in(C.c_void_p(4096 + off), P, P, P, 1, side, None) == INVALID_ARG
            assert b'16-byte aligned' in dry.metro_last_error(), dry.metro_last_error()
    assert dry.metro_last_kernel_id() == b''          # nothing was dispatched


def test_images_u8_to_f32_rejects_bad_arguments(lib):
    assert lib.metro_images_u8_to_f32(None, 16, P, None) == INVALID_ARG
    assert lib.metro_images_u8_to_f32(P, 0, P, None) == INVALID_ARG
    assert b'images_u8_to_f32' in lib.metro_last_error()


@pytest.mark.parametrize('precision', ['f64', 'f32m'])
def test_forward_u8_is_for_f16_plans(lib, precision):
    eng = Engine(ModelSpec(50, 32, 'h36m', base_width=8), None, precision, max_batch=2)
    assert lib.metro_forward_u8(eng._plan, P, 1, P, None, P, None) == INVALID_ARG
    assert b'metro_images_u8_to_f32' in lib.metro_last_error()
    eng.close()


def test_forward_u8_checks_its_pointers(lib):
    eng = Engine(ModelSpec(50, 32, 'h36m', base_width=8), None, 'f16', max_batch=2)
    assert lib.metro_forward_u8(None, P, 1, P, None, P, None) == INVALID_ARG
    assert lib.metro_forward_u8(eng._plan, C.c_void_p(4097), 1, P, None, P, None) == INVALID_ARG
    assert b'16-byte aligned' in lib.metro_last_error()
    assert lib.metro_forward_u8(eng._plan, P, 1, None, None, P, None) == INVALID_ARG
    assert lib.metro_forward_u8(eng._plan, P, 3, P, None, P, None) == INVALID_ARG          # batch > max_batch
    # aligned pointers, nothing bound: the same state error metro_forward gives
    assert lib.metro_forward_u8(eng._plan, P, 1, P, None, P, None) == -4 and b'not bound' in lib.metro_last_error()
    eng.close()


def test_crop_dtype_is_checked_before_any_device_work():
    """No model file, no frames on a device, no GPU: the ValueError comes first."""
    from metro_pose3d_amd.frames import CropParams, estimate_pose_in_frames, locate_poses_in_frames, warp_frames
    frame = np.zeros((8, 8, 3), np.uint8)
    boxes = np.array([[1., 1., 4., 4.]])
    for dtype in ('int8', 'float16', None, np.uint8):
        with pytest.raises(ValueError, match='crop_dtype'):
            estimate_pose_in_frames(frame, boxes, '/nonexistent/model.npz', crop_dtype=dtype)
        with pytest.raises(ValueError, match='crop_dtype'):
            locate_poses_in_frames(frame, boxes, '/nonexistent/model.npz', scale_recovery='metro', crop_dtype=dtype)
        with pytest.raises(ValueError, match='crop_dtype'):
            warp_frames(frame, CropParams(*[np.zeros(0)] * 7), [], crop_dtype=dtype)


def test_cli_crop_dtype_goes_with_frame(capsys):
    from metro_pose3d_amd import inference
    with pytest.raises(SystemExit):
        inference.main(['--model-path', 'm.npz', '--crop-dtype', 'uint8'])
    assert '--crop-dtype goes with --frame' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        inference.main(['--model-path', 'm.npz', '--frame', 'f.npy', '--crop-dtype', 'int8'])


def test_one_multiply_gives_the_fp16_of_the_divide_on_all_256_bytes():
    """The f16 stem kernels compute fp16(rn(float(b) * rn(1 / 255))) where the rule says fp16(rn(float(b) / 255)): the same
    fp16 value for every byte, though the fp32 values differ (so the parity precisions, which use the fp32 value as it is,
    divide)."""
    b = np.arange(256, dtype=np.float32)
    quotient = b / np.float32(255)
    product = b * (np.float32(1) / np.float32(255))
    assert np.array_equal(product.astype(np.float16).view(np.uint16), quotient.astype(np.float16).view(np.uint16))
    assert (product != quotient).any()
