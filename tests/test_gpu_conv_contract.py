"""The MetroConvDesc contract through the C ABI (`-m gpu`): metro_conv_f16 / metro_conv_f64acc / metro_conv_f32m on the
geometries the descriptor states -- rectangular maps, kh != kw, asymmetric and negative TF padding, a pixel stride above
c_in and a channel-slice input, channel tails, fp32 output, rectangular strided residual gathers -- and on both sides of the
dispatcher's shape thresholds, each against the fp64 tap sum tests/helpers.py:ref_conv_desc.

Every case
  * names the kernel family it is meant for and asserts that metro_last_kernel_id() starts with it (a dispatch change cannot
    quietly move the sweep onto the generic kernel; tests/test_conv_contract.py checks the same table by dry runs on the CPU);
  * writes into a NaN-filled output between two 4 KiB guard bands of sentinel bytes: an element never written fails the
    finiteness check, a store outside the tensor (ragged tiles, the c_out % 8 == 4 stores) changes a guard byte;
  * is held to a per-element bound, not a share of the tensor maximum.

The bound.  The fp16 kernels multiply fp16 operands exactly into fp32 and sum K = kh*kw*c_in products plus the bias in fp32,
in an order of their own.  Any order of K + 1 fp32 additions is within (K + 1) * 2^-24 * a of the exact sum, a = sum|w*x| + |b|
(+ |res|) (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 4.4).  So
    fp16 output:  |got - y| <= 2^-10 |y| + 2^-11 |res| + C * 2^-24 * K * a + 2^-24
    fp32 output:  |got - y| <=                            C * 2^-24 * K * a + 2^-24 * 2^-100
2^-10 |y| is twice the half-ulp of the final fp16 rounding; with a residual the conv result is rounded to fp16 once before the
fp16 add (|conv| <= |y| + |res|), which adds 2^-11 (|y| + |res|) at most, covered by the 2^-10 |y| + 2^-11 |res| terms;
2^-24 is the fp16 subnormal spacing (the absolute floor).  C = 8: eight times the worst case of any summation order.  A dropped
tap must fail: a tap of a K-term sum is a / K on average, and C * 2^-24 * K * a < a / K needs C < 2^24 / K^2, = 50.6 at
K = 576 (3x3 x 64 channels); at C = 8 the bound is 1/6 of an average tap, and the 2^-10 |y| term is smaller still (|y| ~ a / sqrt(K)
for random signs).  The precise kernels get the same form with their unit roundoff: fp64 accumulation (2^-53) for
metro_conv_f64acc, fp32 (2^-24) for metro_conv_f32m, and one rounding to the output type (2^-23 |y| for fp32, 2^-52 |y| for fp64)."""
import ctypes as C
import zlib
from dataclasses import dataclass

import numpy as np
import pytest
import torch

from metro_pose3d_amd import _lib
from metro_pose3d_amd._lib import check
from oracle.naive import same_pads
from tests import helpers as H

pytestmark = pytest.mark.gpu

F16, F32, F64 = _lib.METRO_F16, _lib.METRO_F32, _lib.METRO_F64
C_SUM = 8
GUARD = 4096          # bytes of sentinel before and after every output tensor
SENTINEL = 0xA5


@dataclass
class Case:
    name: str
    family: str                 # metro_last_kernel_id() must start with this
    n: int
    h: int
    w: int
    c_in: int
    c_out: int
    kh: int = 3
    kw: int = 3
    stride: int = 1
    dil: int = 1
    pads: tuple = None          # (pad_top, pad_left); default TF SAME
    pix: int = None             # in_pix_stride (default c_in)
    off: int = 0                # channel offset of the input inside its pixel (a channel slice)
    relu: bool = False
    pro: bool = False
    res: tuple = None           # (res_stride, res_offset): residual [n, res_h, res_w, c_out], the smallest that holds the gather
    out: int = F16
    sample: tuple = None        # images the fp64 reference is computed for (default all)

    @property
    def id(self):
        return self.name

    def desc(self, in_dtype=F16, out=None):
        h_out, w_out = -(-self.h // self.stride), -(-self.w // self.stride)
        if self.pads is None:
            pt = same_pads(self.h, (self.kh - 1) * self.dil + 1, self.stride)[0]
            pl = same_pads(self.w, (self.kw - 1) * self.dil + 1, self.stride)[0]
        else:
            pt, pl = self.pads
        rs, ro = self.res or (1, 0)
        return H.conv_desc(self.n, self.h, self.c_in, h_out, self.c_out, 0, self.stride, self.dil, 0, prologue=self.pro,
                           relu=self.relu, residual=self.res is not None, res_h=(h_out - 1) * rs + ro + 1 + (ro > 0),
                           res_w=(w_out - 1) * rs + ro + 1, res_stride=rs, res_offset=ro,
                           out_dtype=self.out if out is None else out, in_dtype=in_dtype, w_in=self.w, w_out=w_out,
                           in_pix_stride=self.pix or self.c_in, kh=self.kh, kw=self.kw, pad_top=pt, pad_left=pl)


DMA, SLAB, C64 = 'conv_igemm_f16_dma<', 'conv3x3_f16_slab<', 'conv3x3_c64'
PW64, PWS, G4 = 'conv_pw64<', 'conv_pws<', 'conv_gemm4w<'

CASES = [
    # ---- rectangular maps on every family
    Case('c64_4x64', C64, 2, 4, 64, 64, 64, relu=True),
    Case('c64_16x8', C64, 4, 16, 8, 64, 64),
    Case('c64_4x32_m512', C64, 4, 4, 32, 64, 64),                     # m = 4 * TN: the smallest c64 layer ...
    Case('c64_4x32_m384', SLAB, 3, 4, 32, 64, 64),                    # ... and one tile less
    Case('slab_12x32_cross_images', SLAB + '64x256', 2, 12, 32, 64, 128, relu=True),
    Case('slab_subgrid_32x64_rate4', SLAB, 1, 32, 64, 64, 128, dil=4),
    Case('slab_capacity_rows512', SLAB + '64x256,rows512', 1, 8, 256, 64, 128, dil=2),
    Case('slab_capacity_rows384', SLAB + '64x256,rows384', 4, 64, 128, 64, 128, dil=2, sample=(0, 3)),
    Case('wide_dilated_4x512', DMA, 1, 4, 512, 64, 64, dil=2),        # used to overflow rows512 (halo 256)
    Case('wide_dilated_8x256_n32', DMA, 32, 8, 256, 64, 128, dil=2, sample=(0, 31)),   # ... rows384 (halo 128)
    Case('wide_dilated_8x256_n128', DMA, 128, 8, 256, 64, 128, dil=2, sample=(0, 64, 127)),   # ... rows640
    Case('dma_7x13', DMA, 2, 7, 13, 64, 128, relu=True),
    Case('pw64_7x13_pro', PW64, 2, 7, 13, 64, 256, 1, 1, pro=True),
    Case('pw64_7x13_res', PW64, 2, 7, 13, 64, 256, 1, 1, res=(1, 0)),
    Case('pw64_7x13_res_sub', PW64, 2, 7, 13, 64, 256, 1, 1, res=(2, 1)),
    Case('pw128_6x10_res', PW64, 3, 6, 10, 128, 512, 1, 1, res=(1, 0)),
    Case('pws_8x12_res', PWS, 2, 8, 12, 256, 1024, 1, 1, res=(1, 0)),
    # ---- gemm4w tile thresholds (1x1 with prologue on 8 x 32 maps): whole / half / quarter tiles, and the ring kernel
    Case('g4_whole_256', G4 + '256x256', 256, 8, 32, 1024, 256, 1, 1, pro=True, sample=(0, 255)),
    Case('g4_half_255', G4 + '256x128', 255, 8, 32, 1024, 256, 1, 1, pro=True, sample=(0, 254)),
    Case('g4_half_112', G4 + '256x128', 112, 8, 32, 1024, 256, 1, 1, pro=True, sample=(0, 111)),
    Case('g4_none_111', DMA, 111, 8, 32, 1024, 256, 1, 1, pro=True, sample=(0, 110)),
    Case('g4_quarter_56', G4 + '256x64', 56, 8, 32, 2048, 256, 1, 1, pro=True, sample=(0, 55)),
    Case('g4_none_55', DMA, 55, 8, 32, 2048, 256, 1, 1, pro=True, sample=(0, 54)),
    # ---- kernel shape kh != kw (generic kernel), with dilation 2 and with stride 2
    Case('k1x3', DMA, 2, 9, 14, 64, 64, 1, 3),
    Case('k3x1_dil2', DMA, 2, 9, 14, 64, 64, 3, 1, dil=2),
    Case('k7x1_s2', DMA, 2, 15, 12, 64, 64, 7, 1, stride=2),
    Case('k1x7_dil2', DMA, 1, 10, 21, 64, 128, 1, 7, dil=2, relu=True),
    Case('k5x3_s2', DMA, 2, 13, 9, 64, 64, 5, 3, stride=2),
    Case('k5x3_dil2', DMA, 1, 12, 11, 64, 136, 5, 3, dil=2),
    # ---- padding: TF SAME at stride 2 on an even x odd map (pad_top 0, pad_left 1), a -1 shift on one axis only
    Case('same_s2_16x15', DMA, 2, 16, 15, 64, 64, stride=2),
    Case('pads_1_0', DMA, 2, 8, 11, 64, 64, pads=(1, 0)),
    Case('shift_-1_0_1x1_s2', DMA, 2, 8, 10, 64, 128, 1, 1, stride=2, pads=(-1, 0)),
    Case('shift_0_-1_1x1_s2', DMA, 2, 8, 10, 64, 128, 1, 1, stride=2, pads=(0, -1)),
    Case('shift_-1_0_3x3', DMA, 1, 9, 8, 64, 64, pads=(-1, 1)),
    # ---- input layout
    Case('pix72', DMA, 2, 7, 9, 64, 64, pix=72),
    Case('pix68', DMA, 2, 7, 9, 64, 64, pix=68),
    Case('pix72_1x1_pro', DMA, 2, 7, 9, 64, 64, 1, 1, pix=72, pro=True),
    Case('slice_off4_pix72', DMA, 2, 7, 9, 64, 64, pix=72, off=4),
    Case('slice_off4_pix68_1x1', DMA, 2, 7, 9, 56, 64, 1, 1, pix=68, off=4),
    # ---- channel counts
    Case('cin8_3x3', DMA + '64x128,bk32', 2, 9, 11, 8, 64),
    Case('cin16_3x3', DMA + '64x128,bk32', 2, 9, 11, 16, 128),
    Case('cin24_3x3_relu', DMA + '64x128,bk32', 2, 9, 11, 24, 64, relu=True),
    Case('cin72_3x3', DMA, 2, 7, 13, 72, 64),
    Case('cin200_3x3', DMA, 1, 7, 13, 200, 128),
    Case('cin2048_1x1', DMA, 1, 5, 6, 2048, 64, 1, 1),
    Case('cin2048_3x3', DMA, 1, 3, 5, 2048, 64),
] + [Case(f'cout{co}_{"f32" if out == F32 else "f16"}', DMA, 2, 7, 13, 64, co, relu=co % 8 == 4, out=out)
     for co in (4, 12, 68, 132, 136) for out in (F16, F32)] + [
    # ---- dispatch thresholds
    Case('slab_m248', DMA, 1, 31, 8, 64, 128),                        # m < 256: not a slab layer ...
    Case('slab_m256', SLAB, 1, 32, 8, 64, 128),                       # ... m = 256: one tile
    Case('slab_blocks128_254', SLAB + '64x256', 127, 16, 16, 64, 256, sample=(0, 63, 126)),
    Case('slab_blocks128_256', SLAB + '128x256', 128, 16, 16, 64, 256, sample=(0, 64, 127)),
    Case('slab_blocks512_254', SLAB + '128x256', 254, 16, 16, 64, 256, sample=(0, 1, 253)),
    Case('slab_blocks512_256', SLAB + '128x512', 256, 16, 16, 64, 256, sample=(0, 1, 255)),
    # ---- residual gathers: res_h != res_w, stride 2, offsets 0 and 1 (generic kernel)
    Case('res_rect_s1', DMA, 2, 7, 6, 96, 136, 1, 1, res=(1, 0)),
    Case('res_rect_s2_off0', DMA, 2, 7, 6, 96, 136, 1, 1, res=(2, 0)),
    Case('res_rect_s2_off1', DMA, 2, 7, 6, 96, 136, 1, 1, res=(2, 1), relu=True),
    Case('res_rect_3x3_s2_off1', DMA, 2, 9, 5, 64, 72, res=(2, 1)),
    Case('res_rect_pw_shape_s2_off0', DMA, 2, 5, 9, 64, 256, 1, 1, stride=2, res=(2, 0)),
]

# the precise kernels: the geometry rows (rectangular, kh != kw, asymmetric pads, pixel stride, residual gather)
PRECISE = [
    Case('p_rect_7x13', '', 2, 7, 13, 24, 20, relu=True),
    Case('p_k5x3_dil2', '', 1, 12, 11, 16, 12, 5, 3, dil=2),
    Case('p_k1x7_s2', '', 2, 9, 16, 8, 8, 1, 7, stride=2),
    Case('p_same_s2_16x15', '', 2, 16, 15, 16, 12, stride=2),
    Case('p_pads_-1_1', '', 1, 9, 8, 12, 8, pads=(-1, 1)),
    Case('p_pix37', '', 2, 7, 9, 30, 16, pix=37),
    Case('p_pix40_off6', '', 2, 7, 9, 30, 16, pix=40, off=6),
    Case('p_res_rect_s2_off1', '', 2, 7, 6, 24, 20, 1, 1, res=(2, 1), relu=True),
    Case('p_res_rect_3x3_s2_off0', '', 2, 9, 5, 16, 12, res=(2, 0)),
]


def _seed(*parts):
    return np.random.default_rng(zlib.crc32('/'.join(map(str, parts)).encode()))


def _operands(case, d, rng):
    """Input buffer [n, h, w, P] (P = in_pix_stride; the kernel reads channels [off, off + c_in) of every pixel), weights,
    bias, prologue, residual."""
    x = rng.standard_normal((d.n, d.h_in, d.w_in, d.in_pix_stride))
    w = rng.standard_normal((d.c_out, d.kh, d.kw, d.c_in)) * np.sqrt(2.0 / (d.kh * d.kw * d.c_in))
    b = rng.standard_normal(d.c_out) * 0.1
    pro = (rng.uniform(0.5, 1.5, d.c_in), rng.standard_normal(d.c_in) * 0.2) if d.has_prologue else None
    res = rng.standard_normal((d.n, d.res_h, d.res_w, d.c_out)) if d.has_residual else None
    return x, w, b, pro, res


def _guarded(shape, dtype, dev):
    """A NaN-filled tensor of `shape` between two GUARD-byte bands of SENTINEL (one allocation); returns (tensor, buffer)."""
    nbytes = int(np.prod(shape)) * torch.tensor([], dtype=dtype).element_size()
    buf = torch.full((GUARD + nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    t = buf[GUARD:GUARD + nbytes].view(dtype).view(shape)
    t.fill_(float('nan'))
    return t, buf


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _input_ptr(t, off):
    return C.c_void_p(t.data_ptr() + off * t.element_size())


def _check(got, y, a, d, u, out_round, res_abs=None, what=''):
    """|got - y| <= out_round |y| (+ out_round / 2 |res|) + C_SUM u K a + floor, element by element (module docstring).
    Returns the worst |got - y| / bound (<= 1)."""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), f'{what}: {int((~np.isfinite(got)).sum())} elements not written (or not finite)'
    k = d.kh * d.kw * d.c_in + 1
    floor = 2.0 ** -24 if d.out_dtype == F16 else 2.0 ** -124
    bound = out_round * np.abs(y) + C_SUM * u * k * a + floor
    if res_abs is not None:
        bound += out_round / 2 * res_abs
    err = np.abs(got - y)
    worst = np.unravel_index(np.argmax(err / bound), err.shape)
    assert (err <= bound).all(), (f'{what}: {int((err > bound).sum())} of {err.size} elements out of bound; worst at {worst}: '
                                  f'got {got[worst]!r} want {y[worst]!r} bound {bound[worst]:.3g} (a {a[worst]:.3g})')
    return float((err / bound).max())


def _sampled(case, d, arrs):
    """The images of the fp64 reference: the descriptor and the per-image arrays restricted to case.sample."""
    if case.sample is None:
        return d, arrs
    import copy
    ds = copy.copy(d)
    ds.n = len(case.sample)
    idx = list(case.sample)
    return ds, [None if t is None else t[idx] for t in arrs]


@pytest.mark.parametrize('case', CASES, ids=[c.id for c in CASES])
def test_conv_f16_contract(lib, cuda, case):
    d = case.desc()
    rng = _seed('f16', case.name)
    x, w, b, pro, res = _operands(case, d, rng)
    x16, w16 = x.astype(np.float16), w.astype(np.float16)
    pro16 = None if pro is None else (pro[0].astype(np.float16), pro[1].astype(np.float16))
    res16 = None if res is None else res.astype(np.float16)
    dev = lambda t, dt: None if t is None else torch.from_numpy(np.ascontiguousarray(t.astype(dt))).to(cuda)
    # (every device tensor is held in a name until the launch has finished: a temporary would return its memory to the
    # caching allocator, which hands it to the next tensor while the kernel still reads it)
    tx, tw, tb = dev(x16, np.float16), dev(w16, np.float16), dev(b, np.float32)
    ts, tsh = dev(pro16 and pro16[0], np.float16), dev(pro16 and pro16[1], np.float16)
    tr = dev(res16, np.float16)
    odt = torch.float16 if d.out_dtype == F16 else torch.float32
    out, buf = _guarded((d.n, d.h_out, d.w_out, d.c_out), odt, cuda)
    check(lib.metro_kernel_notes(1), 'metro_kernel_notes')
    try:
        check(lib.metro_conv_f16(C.byref(d), _input_ptr(tx, case.off), H.ptr(tw), H.ptr(tb), H.ptr(ts), H.ptr(tsh), H.ptr(tr),
                                 H.ptr(out), None), f'metro_conv_f16 {case.name}')
        torch.cuda.synchronize()
        kid = lib.metro_last_kernel_id().decode()
    finally:
        lib.metro_kernel_notes(0)
    assert kid.startswith(case.family), (case.name, kid)
    assert _guards_intact(buf), f'{case.name} ({kid}): a store landed outside the output tensor'
    got = out.cpu().numpy()
    ds, (xs, rs, gs) = _sampled(case, d, [x16[..., case.off:case.off + d.c_in], res16, got])
    y, a = H.ref_conv_desc(ds, xs, w16, b.astype(np.float32), pro=pro16, res=rs)
    rabs = None
    if rs is not None:
        rabs = np.abs(rs.astype(np.float64))[:, d.res_offset::d.res_stride, d.res_offset::d.res_stride][:, :d.h_out, :d.w_out]
    out_round = 2.0 ** -10 if d.out_dtype == F16 else 2.0 ** -23
    _check(gs, y, a, ds, 2.0 ** -24, out_round, rabs, f'{case.name} ({kid})')


def test_f32_output_with_residual_is_refused_and_writes_nothing(lib, cuda):
    # metro_conv_f16's fp32 epilogue has no residual: the combination is refused (include/metro_hip.h), nothing is launched
    case = Case('f32_res', DMA, 2, 7, 13, 64, 128, relu=True, res=(1, 0), out=F32)
    d = case.desc()
    x, w, b, _, res = _operands(case, d, _seed('f32res'))
    dev = lambda t, dt: torch.from_numpy(np.ascontiguousarray(t.astype(dt))).to(cuda)
    tx, tw, tb, tr = dev(x, np.float16), dev(w, np.float16), dev(b, np.float32), dev(res, np.float16)
    out, buf = _guarded((d.n, d.h_out, d.w_out, d.c_out), torch.float32, cuda)
    check(lib.metro_kernel_notes(1), 'metro_kernel_notes')
    try:
        st = lib.metro_conv_f16(C.byref(d), H.ptr(tx), H.ptr(tw), H.ptr(tb), None, None, H.ptr(tr), H.ptr(out), None)
        torch.cuda.synchronize()
        kid = lib.metro_last_kernel_id().decode()
    finally:
        lib.metro_kernel_notes(0)
    assert st != 0 and kid == '' and 'residual' in lib.metro_last_error().decode(), (st, kid)
    assert torch.isnan(out).all() and _guards_intact(buf)


@pytest.mark.parametrize('kernel', ['f64acc_f32', 'f64acc_f64', 'f32m'])
@pytest.mark.parametrize('case', PRECISE, ids=[c.id for c in PRECISE])
def test_precise_conv_contract(lib, cuda, case, kernel):
    io = F64 if kernel == 'f64acc_f64' else F32
    d = case.desc(in_dtype=io, out=io)
    np_io, t_io = (np.float64, torch.float64) if io == F64 else (np.float32, torch.float32)
    np_w = np.float32 if kernel == 'f32m' else np.float64
    x, w, b, _, res = _operands(case, d, _seed(kernel, case.name))
    x, w, b = x.astype(np_io), w.astype(np_w), b.astype(np_w)
    res = None if res is None else res.astype(np_io)
    dev = lambda t: None if t is None else torch.from_numpy(np.ascontiguousarray(t)).to(cuda)
    tx, tw, tb, tr = dev(x), dev(w), dev(b), dev(res)
    out, buf = _guarded((d.n, d.h_out, d.w_out, d.c_out), t_io, cuda)
    fn = lib.metro_conv_f32m if kernel == 'f32m' else lib.metro_conv_f64acc
    check(fn(C.byref(d), _input_ptr(tx, case.off), H.ptr(tw), H.ptr(tb), None, None, H.ptr(tr), H.ptr(out), None),
          f'{kernel} {case.name}')
    torch.cuda.synchronize()
    assert _guards_intact(buf), f'{kernel} {case.name}: a store landed outside the output tensor'
    y, a = H.ref_conv_desc(d, x[..., case.off:case.off + d.c_in], w, b, res=res)
    u = 2.0 ** -24 if kernel == 'f32m' else 2.0 ** -53
    _check(out.cpu().numpy(), y, a, d, u, 2.0 ** -23 if io == F32 else 2.0 ** -52, what=f'{kernel} {case.name}')
