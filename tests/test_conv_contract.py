"""The contract of metro_conv_f16 (include/metro_hip.h MetroConvDesc) on the CPU: the general fp64 reference the GPU
contract sweep (tests/test_gpu_conv_contract.py) compares with, checked against the other references and a hand-computed
answer; and DRY RUNS of the dispatcher (metro_kernel_notes(2): the entry point records the kernel it would launch and
launches nothing), which show that every shape predicate hands a layer only to a kernel that can hold it, and that the
limits the header states are refused before any launch."""
import ctypes as C
import re
import zlib

import numpy as np
import pytest

from metro_pose3d_amd import _lib
from oracle import naive
from tests import helpers as H

F16, F32 = _lib.METRO_F16, _lib.METRO_F32


# ---- the reference ------------------------------------------------------------------------------------------------------

def _operands(rng, d, pix=None):
    x = rng.standard_normal((d.n, d.h_in, d.w_in, pix or d.c_in))
    w = rng.standard_normal((d.c_out, d.kh, d.kw, d.c_in))
    b = rng.standard_normal(d.c_out)
    return x, w, b


# (n, h_in, c_in, h_out, c_out, k, stride, dil, pad): square maps and kernels, where ref_conv_nhwc applies
SQUARE = [(2, 9, 3, 9, 4, 3, 1, 1, 1), (1, 8, 2, 4, 3, 3, 2, 1, 0), (1, 8, 2, 4, 3, 3, 2, 1, 1), (2, 12, 2, 12, 2, 3, 1, 2, 2),
          (1, 7, 3, 4, 2, 1, 2, 1, -1), (1, 10, 2, 5, 2, 5, 2, 1, 2), (1, 6, 2, 6, 5, 1, 1, 1, 0)]


# (a prologue is defined for un-padded 1x1 convolutions only)
SQUARE_VARIANTS = [(c, v) for c in SQUARE for v in ('plain', 'relu', 'prologue', 'residual')
                   if v != 'prologue' or (c[5] == 1 and c[8] <= 0)]


@pytest.mark.parametrize('case,variant', SQUARE_VARIANTS, ids=[f'{c}-{v}' for c, v in SQUARE_VARIANTS])
def test_ref_conv_desc_matches_ref_conv_nhwc(case, variant):
    n, h_in, c_in, h_out, c_out, k, stride, dil, pad = case
    rng = np.random.default_rng(zlib.crc32(f'{case}/{variant}'.encode()))
    res_stride, res_off = (2, 1) if h_out * 2 + 1 <= 2 * h_in else (1, 0)
    res_h = (h_out - 1) * res_stride + res_off + 1
    d = H.conv_desc(n, h_in, c_in, h_out, c_out, k, stride, dil, pad, prologue=variant == 'prologue', relu=variant == 'relu',
                    residual=variant == 'residual', res_h=res_h, res_stride=res_stride, res_offset=res_off)
    x, w, b = _operands(rng, d)
    pro = (rng.uniform(0.5, 1.5, c_in), rng.standard_normal(c_in)) if variant == 'prologue' else None
    res = rng.standard_normal((n, res_h, res_h, c_out)) if variant == 'residual' else None
    y, a = H.ref_conv_desc(d, x, w, b, pro=pro, pro_round=None, res=res)
    ref = H.ref_conv_nhwc(x, w, b, stride, dil, pad, h_out, pro=pro, relu=variant == 'relu', res=res,
                          res_stride=res_stride, res_offset=res_off).numpy()
    np.testing.assert_allclose(y, ref, rtol=1e-12, atol=1e-12)
    assert (a >= np.abs(y) - 1e-12).all()


# (n, h, w, c_in, c_out, k, stride, rate, pad_beg, pad_end): oracle/naive.py's explicit zero padding (square kernels, the
# same pad on both axes) on rectangular maps
NAIVE = [(1, 7, 12, 3, 2, 3, 1, 1, 1, 1), (2, 10, 5, 2, 3, 3, 2, 1, 0, 1), (1, 9, 14, 2, 2, 3, 1, 2, 2, 2), (1, 11, 6, 2, 2, 5, 2, 1, 2, 2),
         (1, 6, 9, 3, 2, 1, 2, 1, 0, 0)]


@pytest.mark.parametrize('case', NAIVE, ids=[str(c) for c in NAIVE])
def test_ref_conv_desc_matches_oracle_naive(case):
    n, h, wd, c_in, c_out, k, stride, rate, pb, pe = case
    rng = np.random.default_rng(zlib.crc32(str(case).encode()))
    x = rng.standard_normal((n, h, wd, c_in))
    w_hwio = rng.standard_normal((k, k, c_in, c_out))
    ref = naive.conv_nhwc(x, w_hwio, stride, rate, pb, pe)
    d = H.conv_desc(n, h, c_in, ref.shape[1], c_out, k, stride, rate, pb, w_in=wd, w_out=ref.shape[2])
    y, _ = H.ref_conv_desc(d, x, w_hwio.transpose(3, 0, 1, 2), np.zeros(c_out))
    np.testing.assert_allclose(y, ref, rtol=1e-12, atol=1e-12)


def test_ref_conv_desc_hand_computed_negative_pad_1x2():
    # x[0, :, :, 0] = [[0 1 2 3] [4 5 6 7] [8 9 10 11]]; 1x2 kernel [1, 10]; pad_top -1 (row 0 skipped), pad_left 1 (column -1
    # reads zero): y[ho, wo] = x[ho + 1, wo - 1] + 10 x[ho + 1, wo] + 0.5; the residual [1, 3, 5] is gathered at stride 1 offset 1
    d = H.conv_desc(1, 3, 1, 2, 1, 1, w_in=4, w_out=4, kh=1, kw=2, pad_top=-1, pad_left=1, residual=True, res_h=3, res_w=5,
                    res_offset=1)
    x = np.arange(12.0).reshape(1, 3, 4, 1)
    w = np.array([1.0, 10.0]).reshape(1, 1, 2, 1)
    res = np.arange(15.0).reshape(1, 3, 5, 1) * 100
    y, a = H.ref_conv_desc(d, x, w, [0.5], res=res)
    conv = np.array([[40, 54, 65, 76], [80, 98, 109, 120]]) + 0.5
    gathered = np.array([[600, 700, 800, 900], [1100, 1200, 1300, 1400]])
    np.testing.assert_array_equal(y[0, :, :, 0], conv + gathered)
    np.testing.assert_array_equal(a[0, :, :, 0], conv + gathered)          # every term is positive here


def test_ref_conv_desc_pixel_stride_and_prologue_rounding():
    rng = np.random.default_rng(7)
    d = H.conv_desc(1, 5, 8, 5, 3, 1, prologue=True, w_in=6, w_out=6, in_pix_stride=12)
    x = rng.standard_normal((1, 5, 6, 12))
    w, b = rng.standard_normal((3, 1, 1, 8)), rng.standard_normal(3)
    sc, sh = rng.uniform(0.5, 1.5, 8), rng.standard_normal(8)
    y, _ = H.ref_conv_desc(d, x, w, b, pro=(sc, sh))
    xin = np.maximum((x[..., :8] * sc + sh).astype(np.float16).astype(np.float64), 0)
    np.testing.assert_allclose(y, xin @ w[:, 0, 0].T + b, rtol=1e-12, atol=1e-12)


# ---- dry runs of the dispatcher -----------------------------------------------------------------------------------------

_P = C.c_void_p(4096)     # any non-NULL pointer: a dry run launches nothing


@pytest.fixture()
def dry(lib):
    lib.metro_kernel_notes(2)
    yield lib
    lib.metro_kernel_notes(0)


def _dispatch(lib, d):
    """(status, kernel id) of metro_conv_f16 on `d` without launching."""
    lib.metro_kernel_notes(2)          # clears the id
    st = lib.metro_conv_f16(C.byref(d), _P, _P, _P, _P, _P, _P, _P, None)
    return st, lib.metro_last_kernel_id().decode()


def _same3x3(n, h, w, c_in, c_out, rate):
    return H.conv_desc(n, h, c_in, h, c_out, 3, 1, rate, rate, w_in=w, w_out=w, in_dtype=F16)


_SLAB = re.compile(r'conv3x3_f16_slab<(\d+)x(\d+),rows(\d+),[^>]*>(\+subgrid)?$')


def _slab_fits(d, kid):
    """None if `kid` is not the slab kernel, else (halo the layer needs, halo the named configuration holds)."""
    m = _SLAB.match(kid)
    if m is None:
        return None
    tn, rows, sub = int(m.group(2)), int(m.group(3)), m.group(4) is not None
    halo = d.w_out // d.dilation if sub else d.dilation * d.w_out
    return halo, (rows - tn) // 2


def _threshold_batches(hw, c_out):
    """Batches around the slab launcher's tile-count thresholds (blocks128 < 256 -> 64-cout tiles; blocks512 >= 256 ->
    512-pixel tiles), and the first batch with m >= 256 pixels."""
    t = (c_out + 127) // 128
    ns = {1, 2}
    for px in (256, 512):
        n = next((n for n in range(1, 4097) if t * ((n * hw + px - 1) // px) >= 256), None)
        if n is not None:
            ns |= {n - 1, n}
    n256 = -(-256 // hw)
    ns |= {n256 - 1, n256}
    return sorted(n for n in ns if n >= 1)


def test_slab_never_gets_a_halo_its_slab_cannot_hold(dry):
    # 3x3 stride-1 SAME fp16 layers over map widths (powers of two and not), heights, rates, channels and batches across both
    # tile-count thresholds: every layer dispatched to the tap-reuse slab kernel must fit its slab, (rows - TN) / 2 rows of halo
    widths = [8, 16, 24, 32, 48, 64, 96, 128, 192, 256, 320, 512, 1024]
    seen_slab, seen_sub = set(), set()
    bad = []
    for wd in widths:
        for h in sorted({wd, 4, 8, 2 * wd}):
            for rate in range(1, 9):
                for c_in in (64, 128, 256):
                    for c_out in (64, 128, 256):
                        for n in _threshold_batches(h * wd, c_out):
                            d = _same3x3(n, h, wd, c_in, c_out, rate)
                            st, kid = _dispatch(dry, d)
                            assert st == 0 and kid, (n, h, wd, c_in, c_out, rate, st)
                            fit = _slab_fits(d, kid)
                            if fit is None:
                                continue
                            (seen_sub if kid.endswith('+subgrid') else seen_slab).add(kid.split('>')[0])
                            if fit[0] > fit[1]:
                                bad.append(((n, h, wd, c_in, c_out, rate), kid, fit))
    assert not bad, f'{len(bad)} layers on a slab too small for their halo (layer, id, (halo, holds)), e.g. {bad[:8]}'
    # the sweep reached every slab configuration in both pixel orders (it tests the predicate, not an empty set)
    assert len(seen_slab) >= 8 and len(seen_sub) >= 4, (sorted(seen_slab), sorted(seen_sub))


# (n, h, w, c_in, c_out, rate) -> the kernel family that must run it
WIDE_DILATED = [
    # halo W/d past the configuration the launcher would pick: the generic ring kernel
    ((1, 4, 512, 64, 64, 2), 'conv_igemm_f16_dma<'),        # halo 256 vs rows512's 128
    ((32, 8, 256, 64, 128, 2), 'conv_igemm_f16_dma<'),      # halo 128 vs rows384's 64
    ((128, 8, 256, 64, 128, 2), 'conv_igemm_f16_dma<'),     # halo 128 vs rows640 (512-pixel tiles)'s 64
    ((2, 256, 256, 64, 128, 2), 'conv_igemm_f16_dma<'),
    ((1, 256, 256, 128, 128, 2), 'conv_igemm_f16_dma<'),    # halo 128 vs rows384's 64
    # exactly at capacity: stay on the slab
    ((1, 8, 256, 64, 128, 2), 'conv3x3_f16_slab<64x256,rows512,'),
    ((4, 64, 128, 64, 128, 2), 'conv3x3_f16_slab<64x256,rows384,'),
]


@pytest.mark.parametrize('case,family', WIDE_DILATED, ids=[str(c[0]) for c in WIDE_DILATED])
def test_wide_dilated_maps_dispatch(dry, case, family):
    d = _same3x3(*case)
    st, kid = _dispatch(dry, d)
    assert st == 0 and kid.startswith(family), (case, st, kid)
    fit = _slab_fits(d, kid)
    assert fit is None or fit[0] <= fit[1], (case, kid, fit)


def test_f32_output_with_residual_is_rejected(dry):
    # conv_igemm_f16_dma's fp32 epilogue (the only fp32-output one) has no residual: the entry refuses the combination
    for case in [(2, 16, 16, 64, 128, 1, 1), (2, 7, 13, 72, 136, 3, 1), (1, 8, 8, 64, 64, 1, 2)]:
        n, h, w, c_in, c_out, k, stride = case
        h_out, w_out = -(-h // stride), -(-w // stride)
        d = H.conv_desc(n, h, c_in, h_out, c_out, k, stride, 1, (k - 1) // 2, w_in=w, w_out=w_out, residual=True, res_h=h,
                        res_w=w, res_stride=stride, relu=True, out_dtype=F32, in_dtype=F16)
        st, kid = _dispatch(dry, d)
        assert st != 0 and kid == '', (case, st, kid)
        assert 'residual' in dry.metro_last_error().decode(), dry.metro_last_error()
        # ... and the same layer without the residual, or with fp16 output, is served
        d.has_residual = 0
        assert _dispatch(dry, d)[0] == 0
        d.has_residual, d.out_dtype = 1, F16
        assert _dispatch(dry, d)[0] == 0


def _reject_cases():
    ok = dict(n=2, h_in=8, c_in=64, h_out=8, c_out=64, k=3, pad=1, in_dtype=F16)
    return [
        ('c_in % 8', dict(ok, c_in=12, in_pix_stride=12)),
        ('c_in % 8 (1x1)', dict(ok, c_in=36, k=1, pad=0)),
        ('c_in > 2048', dict(ok, c_in=2056)),
        ('c_in > 2048 (slab shape)', dict(ok, n=8, h_in=16, h_out=16, c_in=4096)),
        ('c_in > 2048 (1x1)', dict(ok, c_in=4096, c_out=256, k=1, pad=0, prologue=True)),
        ('c_out % 4', dict(ok, c_out=66)),
        ('c_out % 4 (1x1)', dict(ok, c_out=6, k=1, pad=0)),
        ('c_out % 8 with residual', dict(ok, c_out=68, residual=True, res_h=8)),
        ('c_out % 8 with residual (1x1)', dict(ok, c_out=12, k=1, pad=0, residual=True, res_h=8)),
        ('residual gather out of bounds', dict(ok, residual=True, res_h=8, res_offset=1)),
        ('residual gather out of bounds (stride)', dict(ok, residual=True, res_h=14, res_stride=2)),
        ('residual width out of bounds', dict(ok, residual=True, res_h=8, res_w=7)),
        ('prologue with padding', dict(ok, k=1, pad=1, h_out=10, prologue=True)),
        ('prologue on a 3x3', dict(ok, prologue=True)),
        ('prologue reading past the end', dict(ok, k=1, pad=-1, prologue=True)),
        ('in_pix_stride % 4', dict(ok, in_pix_stride=66)),
        ('in_dtype F32', dict(ok, in_dtype=F32)),
    ]


@pytest.mark.parametrize('what,kw', _reject_cases(), ids=[c[0] for c in _reject_cases()])
def test_stated_limits_are_rejected_without_a_launch(dry, what, kw):
    kw = dict(kw)
    d = H.conv_desc(kw.pop('n'), kw.pop('h_in'), kw.pop('c_in'), kw.pop('h_out'), kw.pop('c_out'), kw.pop('k'), **kw)
    st, kid = _dispatch(dry, d)
    assert st != 0 and kid == '', (what, st, kid)
    assert dry.metro_last_error().decode(), what


def test_reject_cases_are_one_step_from_accepted_layers(dry):
    # the base layer of the rejection cases and its nearest legal neighbours are served (a rejection test that every
    # descriptor fails proves nothing)
    for kw in [dict(c_in=64), dict(c_in=2048), dict(c_in=16, in_pix_stride=16), dict(c_out=68), dict(c_out=72, residual=True, res_h=8),
               dict(residual=True, res_h=15, res_stride=2, h_out=8), dict(in_pix_stride=68)]:
        base = dict(n=2, h_in=8, c_in=64, h_out=8, c_out=64, k=3, pad=1, in_dtype=F16)
        base.update(kw)
        d = H.conv_desc(base.pop('n'), base.pop('h_in'), base.pop('c_in'), base.pop('h_out'), base.pop('c_out'), base.pop('k'), **base)
        st, kid = _dispatch(dry, d)
        assert st == 0 and kid, (kw, st, dry.metro_last_error())


def test_gpu_contract_sweep_dispatches_to_its_families(dry):
    # the case table of tests/test_gpu_conv_contract.py by dry runs: each case reaches the kernel family it is meant for, so a
    # dispatch change that moves a case shows here first (the GPU test asserts the same on the launch it makes)
    from tests.test_gpu_conv_contract import CASES
    for case in CASES:
        st, kid = _dispatch(dry, case.desc())
        assert st == 0 and kid.startswith(case.family), (case.name, st, kid, dry.metro_last_error())
        fit = _slab_fits(case.desc(), kid)
        assert fit is None or fit[0] <= fit[1], (case.name, kid, fit)


# ---- the fused entry points by dry runs ---------------------------------------------------------------------------------
# metro_conv_f16_pair / _next / _next_proj / _next_rebuild / _gemm4w: each accepted form reaches its kernel, and a layer one
# step off a shape rule (pair split, c2, map width of the rebuilt residual, sub_off, whole gemm4w tiles) is refused with its
# status and without a launch

def _fused(lib, entry, d, split=0, c2=64, out=True, out_sub=False, sub_off=0, classic=False):
    """(status, kernel id) of one fused entry point on `d` without launching; classic = under metro_conv_b1_form(1)."""
    p, o = _P, (_P if out else None)
    lib.metro_kernel_notes(2)
    lib.metro_conv_b1_form(int(classic))
    try:
        if entry == 'pair':
            st = lib.metro_conv_f16_pair(C.byref(d), p, p, p, p, p, o, split, p, None)
        elif entry == 'next':
            st = lib.metro_conv_f16_next(C.byref(d), p, p, p, p, o, p, p, p, p, p, c2, None)
        elif entry == 'next_proj':
            st = lib.metro_conv_f16_next_proj(C.byref(d), p, p, p, p, p, p, p, p, o, p, p, p, p, p, c2, None)
        elif entry == 'next_rebuild':
            st = lib.metro_conv_f16_next_rebuild(C.byref(d), p, p, p, p, p, p, p, p, p, p, p, o, _P if out_sub else None, sub_off,
                                                 p, p, p, p, p, c2, None)
        else:
            st = lib.metro_conv_f16_gemm4w(C.byref(d), p, p, p, p, p, p, o, split, _P if split else None, None)
    finally:
        lib.metro_conv_b1_form(0)
    return st, lib.metro_last_kernel_id().decode()


def _pw(n, side, c_in, c_out, w=None, **kw):
    """A 1x1 stride-1 fp16 layer on an n x side x w map."""
    return H.conv_desc(n, side, c_in, side, c_out, 1, w_in=w, w_out=w, in_dtype=F16, **kw)


_RES = dict(residual=True, res_h=16)

# (name, entry, desc, call arguments, kernel id)
FUSED_ACCEPTED = [
    ('pair block1', 'pair', _pw(2, 16, 64, 320, prologue=True), dict(split=256), 'conv_pw64<k64,wm4,pro,pair>'),
    ('pair block2', 'pair', _pw(2, 16, 256, 640, prologue=True), dict(split=512), 'conv_pw64<k256,wm8,cb512,pro,pair>'),
    ('pair block2 classic', 'pair', _pw(2, 16, 256, 640, prologue=True), dict(split=512, classic=True),
     'conv_igemm_f16_dma<128x128,bk64,s2,pro>+pair'),
    ('pair block3', 'pair', _pw(2, 16, 512, 1280, prologue=True), dict(split=1024), 'conv_igemm_f16_dma<128x128,bk64,s2,pro>+pair'),
    ('pair block4 batch 128', 'pair', _pw(128, 8, 1024, 2560, prologue=True), dict(split=2048), 'conv_gemm4w<256x256,pro>+pair'),
    ('pair 256 + 72', 'pair', _pw(2, 16, 64, 328, prologue=True), dict(split=256), 'conv_igemm_f16_dma<128x128,bk64,s1,pro>+pair'),
    ('next block1', 'next', _pw(2, 16, 64, 256, **_RES), dict(c2=64), 'conv_pw64<k64,wm4,res,next>'),
    ('next block2', 'next', _pw(2, 16, 128, 512, **_RES), dict(c2=128), 'conv_pw64<k128,wm8,cb512,res,next>'),
    ('next without residual', 'next', _pw(2, 16, 64, 256), dict(c2=64), 'conv_igemm_f16_fuse2<256x64>'),
    ('next_proj', 'next_proj', _pw(2, 16, 64, 256), dict(), 'conv_pw64<k64,wm4,next,projsc>'),
    ('next_proj on chip', 'next_proj', _pw(2, 16, 64, 256), dict(out=False), 'conv_b1_chain<projsc,noout>'),
    ('next_proj on chip classic', 'next_proj', _pw(2, 16, 64, 256), dict(out=False, classic=True),
     'conv_pw64<k64,wm4,next,projsc,noout>'),
    ('next_proj on chip width 8', 'next_proj', _pw(2, 8, 64, 256), dict(out=False), 'conv_pw64<k64,wm4,next,projsc,noout>'),
    ('next_rebuild', 'next_rebuild', _pw(2, 16, 64, 256), dict(), 'conv_b1_chain<rebuild>'),
    ('next_rebuild sub', 'next_rebuild', _pw(2, 16, 64, 256), dict(out=False, out_sub=True), 'conv_b1_chain<rebuild,subout>'),
    ('next_rebuild sub 1', 'next_rebuild', _pw(2, 16, 64, 256), dict(out=False, out_sub=True, sub_off=1), 'conv_b1_chain<rebuild,subout>'),
    ('next_rebuild classic', 'next_rebuild', _pw(2, 16, 64, 256), dict(classic=True), 'conv_pw64<k64,wm4,next,projsc,rebuild>'),
    ('next_rebuild sub classic', 'next_rebuild', _pw(2, 16, 64, 256), dict(out=False, out_sub=True, classic=True),
     'conv_pw64<k64,wm4,next,projsc,rebuild,subout>'),
    ('gemm4w', 'gemm4w', _pw(2, 16, 512, 256, prologue=True), dict(), 'conv_gemm4w<256x256,pro>'),
    ('gemm4w pair', 'gemm4w', _pw(2, 16, 1024, 2560, prologue=True), dict(split=2048), 'conv_gemm4w<256x256,pro>+pair'),
]

# (name, entry, desc, call arguments, status): each one step off an accepted case above
FUSED_REJECTED = [
    ('pair split % 256', 'pair', _pw(2, 16, 64, 320, prologue=True), dict(split=100), -1),
    ('pair second output % 8', 'pair', _pw(2, 16, 64, 324, prologue=True), dict(split=256), -1),
    ('pair with residual', 'pair', _pw(2, 16, 64, 320, prologue=True, **_RES), dict(split=256), -1),
    ('next block1 c2 128', 'next', _pw(2, 16, 64, 256, **_RES), dict(c2=128), -1),
    ('next block2 c2 64', 'next', _pw(2, 16, 128, 512, **_RES), dict(c2=64), -1),
    ('next c_out 128', 'next', _pw(2, 16, 64, 128, **_RES), dict(c2=64), -1),
    ('next_proj c2 128', 'next_proj', _pw(2, 16, 64, 256), dict(c2=128), -1),
    ('next_proj with residual', 'next_proj', _pw(2, 16, 64, 256, **_RES), dict(), -1),
    ('next_rebuild width 24', 'next_rebuild', _pw(2, 16, 64, 256, w=24), dict(), -1),
    ('next_rebuild width 8', 'next_rebuild', _pw(2, 8, 64, 256), dict(), -1),
    ('next_rebuild c2 128', 'next_rebuild', _pw(2, 16, 64, 256), dict(c2=128), -1),
    ('next_rebuild sub_off 2', 'next_rebuild', _pw(2, 16, 64, 256), dict(out=False, out_sub=True, sub_off=2), -1),
    ('next_rebuild both outputs', 'next_rebuild', _pw(2, 16, 64, 256), dict(out_sub=True), -1),
    ('next_rebuild no output', 'next_rebuild', _pw(2, 16, 64, 256), dict(out=False), -1),
    ('gemm4w partial tile', 'gemm4w', _pw(1, 8, 512, 256), dict(), -2),
    ('gemm4w pair second output % 256', 'gemm4w', _pw(2, 16, 1024, 2176, prologue=True), dict(split=2048), -2),
]


@pytest.mark.parametrize('name,entry,d,kw,kid', FUSED_ACCEPTED, ids=[c[0] for c in FUSED_ACCEPTED])
def test_fused_entries_reach_their_kernels(dry, name, entry, d, kw, kid):
    st, got = _fused(dry, entry, d, **kw)
    assert (st, got) == (0, kid), (name, st, got, dry.metro_last_error())


@pytest.mark.parametrize('name,entry,d,kw,status', FUSED_REJECTED, ids=[c[0] for c in FUSED_REJECTED])
def test_fused_entries_reject_shapes_one_step_off(dry, name, entry, d, kw, status):
    st, got = _fused(dry, entry, d, **kw)
    assert (st, got) == (status, ''), (name, st, got)
    assert dry.metro_last_error().decode(), name
