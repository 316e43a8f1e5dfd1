"""IEEE special values through the C ABI, one kernel family at a time (`-m gpu`).

The f16 path promises that a crop which cannot be computed in fp16 storage is reported, not answered: the finalize launch
screens the soft-argmax statistics.  That only works if every launch in front of it treats a non-finite value the way IEEE
arithmetic on its fp64 restatement does.  The contract (include/metro_hip.h, MetroConvDesc):

    relu(NaN) = NaN      relu(+Inf) = +Inf      relu(-Inf) = 0      a store past the largest fp16 (65 504) is +-Inf

and a non-finite element reaches exactly the outputs it is a term of.  -Inf -> 0 is deliberate: the value behind a -Inf is hugely
negative, zero is its ReLU.  The reference is the fp64 restatement the other kernel tests use (tests/helpers.py:ref_conv_desc,
the prologue as one fp16 FMA, fp16 roundings by astype(np.float16), which gives inf on overflow), evaluated with IEEE special
values under np.errstate(all='ignore'); its ReLU is np.maximum, which propagates NaN.

Every case (NF_CASES; tests/test_kernel_coverage.py checks without a GPU, by dry runs, that each case launches exactly the ids it
names and that every kernel of its configurations is launched by one -- the three kernels of head_f16.hip and the two of
stem_pool_f16.hip counted apart; the experimental GEMM forms of libmetro_experimental.so, which no plan dispatches, have cases
too) asserts first that no weight, bias, scale or shift is zero
(Inf * 0), then runs

  1. the clean launch: every element finite and within the bound of the case's own existing test;
  2. +Inf, -Inf and NaN at one input element, at each of: pixel (0, 0) channel 0; the last pixel of the last image, last
     channel; a middle channel of the pixel in front of the first pixel-tile boundary (flat pixel 63, or 255 where the map has
     256 pixels).  One plant per image and launch, so the images of a batch never share one; as many launches as that takes;
  3. where the entry point reads one, the same three values at one element of the residual tensor / the shortcut's input;
  4. store overflow from finite data (launches that store fp16): one input element 1024 and the weights of one output channel
     on its input channel 512, of another -512, so that those outputs are >= 2 * 65504 in magnitude and every other value the
     launch rounds to fp16 is <= 0.5 * 65504.  That gap is asserted on the reference: a condition on the inputs, not a
     tolerance.  +-Inf is expected at exactly the first set.  (fp32 and fp64 stores do not overflow at any magnitude these
     layers see: the precise kernels and the fp32 logits get no such plant.)
  5. poisoned surroundings: every input of the launch lives in ONE allocation, each between two 4 KiB bands; the launch with
     the bands (and, for a channel-slice input, the channels of each pixel outside the slice) holding NaN must give the bits
     of the launch with zeros there.  A boundary mask applied as a multiply, or a K tail padded with zero weights over
     whatever lies behind the tensor, shows only when that garbage is NaN.  Everything read stays inside the allocation.

and asserts for every output of every planted launch

  * class equality with the reference at EVERY element: finite, +Inf, -Inf or NaN.  The plants are single elements, so no class
    depends on the summation order (a sum holding +Inf and -Inf is NaN in any order);
  * elements the plant cannot influence -- equal in the clean and the planted reference and finite in both; every other image
    of the batch is among them -- carry the bits of the clean launch;
  * influenced but finite elements (behind a -Inf -> 0) stay within the bound of the case's existing test: the per-element
    bound of the conv-contract table, 2e-3 of the layer maximum (over its finite elements) for the fused launches.

The soft-argmax outputs (poses) are held to the same three: a NaN or +Inf logit makes its joint's exact soft-argmax NaN (every
joint's, if the joint is the root), a -Inf logit has weight zero.  The status word that reports such a crop exists in the plan's
workspace only: tests/test_gpu_nonfinite_screen.py holds it on whole forwards.  metro_stem_pool_f32in gets the store-overflow
plant only: a non-finite image is the caller's error, and the pool's max over a -Inf is that of the finite values beside it."""
import copy
import ctypes as C
import zlib
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from metro_pose3d_amd import ModelSpec, _lib
from metro_pose3d_amd._lib import check
from tests import helpers as H
from tests import test_gpu_conv_contract as CC
from tests.test_gpu_kernels import CONV_CASES, G8_CASES

pytestmark = pytest.mark.gpu

F16, F32, F64 = _lib.METRO_F16, _lib.METRO_F32, _lib.METRO_F64
f16, f32, f64 = np.float16, np.float32, np.float64
BAND = 4096                     # bytes in front of and behind every input tensor
F16_MAX = 65504.0
NAN_BITS = {2: np.uint16(0x7E00), 4: np.uint32(0x7FC00000), 8: np.uint64(0x7FF8000000000000)}
UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}
TORCH = {np.dtype(f16): torch.float16, np.dtype(f32): torch.float32, np.dtype(f64): torch.float64}
SPECIALS = (np.inf, -np.inf, np.nan)
BIG_X, BIG_W = 1024.0, 512.0    # the store-overflow plant: 1024 * (0.5 .. 1.5) * 512 >= 2 * 65504 behind any prologue scale
_DRY = C.c_void_p(4096)         # any non-NULL pointer: a dry run launches nothing


@dataclass
class NFCase:
    name: str
    families: tuple             # the launches' kernel ids, in order, must start with these
    kind: str
    arg: object

    @property
    def id(self):
        return f'{self.kind}-{self.name}'

    def family_names(self):
        return {kernel_of(f) for f in self.families}

    def problem(self):
        return _BUILDERS[self.kind](self.arg)


# ---- the reference's pieces (IEEE special values pass through all of them) ------------------------------------------------
def _r(a, dt):
    """One rounding to `dt` (inf past its range), back in fp64."""
    return np.asarray(a).astype(dt).astype(f64)


def _pre(x, sc, sh, dt=f16):
    """The prologue: relu(x * scale + shift), one rounding to `dt` (the kernels' FMA); NaN stays NaN, +Inf stays +Inf."""
    v = np.asarray(x, f64) * np.asarray(sc, f64) + np.asarray(sh, f64)
    return np.maximum(v if dt is None else _r(v, dt), 0.0)


def _mm(x, w, b):
    """1x1 convolution + bias in fp64: x [..., K], w [O, K] (or [O, 1, 1, K])."""
    w = np.asarray(w, f64)
    return np.asarray(x, f64) @ w.reshape(w.shape[0], -1).T + np.asarray(b, f64)


def _out(stored, exact, bound=None, rel=2e-3):
    """One output of the reference: what the kernel stores (classes, fp64 of the rounded value), the exact value, and the
    per-element bound on |got - exact| -- by default `rel` of the layer maximum over its finite elements."""
    if bound is None:
        fin = np.isfinite(exact)
        bound = np.full(exact.shape, rel * (np.abs(exact[fin]).max() if fin.any() else 0.0))
    return SimpleNamespace(stored=stored, exact=exact, bound=bound)


def _rng(*parts):
    return np.random.default_rng(zlib.crc32(('nonfinite/' + '/'.join(map(str, parts))).encode()))


def _nz(a):
    """`a` with its zeros (a small draw rounded to fp16) replaced by the smallest normal number: Inf * 0 is not a plant's business."""
    a[a == 0] = np.finfo(a.dtype).tiny
    return a


def _he(rng, c_out, c_in, k=1, gain=1.0):
    return _nz((rng.standard_normal((c_out, k, k, c_in)) * np.sqrt(2.0 / (k * k * c_in)) * gain).astype(f16))


def _pro(rng, c, dt=f16):
    return rng.uniform(0.5, 1.5, c).astype(dt), _nz((rng.standard_normal(c) * 0.2).astype(dt))


def _ptr(p, name):
    return p.get(name) or C.c_void_p(0)


class Problem:
    """One launch (or chain of launches) and its reference.
    tensors   name -> numpy array of the device dtype: every input, in the order they are laid out in the allocation
    batched   names whose first axis is the image
    x         (name, channel offset, c_in) of the input [n, h, w, P] that takes the plants
    res       None, or (name, stride, offset, h_out, w_out) of the tensor [n, rh, rw, c] whose pixel
              (oh * stride + offset, ow * stride + offset) output pixel (oh, ow) reads
    outs      [(shape, numpy dtype)] of the outputs
    launch    (lib, p: name -> c_void_p, o: [c_void_p], scratch c_void_p) -> None
    ref       (t: name -> numpy array, the batched ones restricted to `sample`) -> ([_out per output], [every fp64 array the
              launch rounds to fp16])
    overflow  None, or [(name, index, value)]: the store-overflow plant
    unused    name -> boolean mask (broadcastable) of elements inside a tensor that the launch must never use
    nonzero   names of the parameters asserted free of zeros
    reads     (row, column) -> whether the launch reads that pixel of x at all"""

    def __init__(self, n, tensors, batched, x, outs, launch, ref, nonzero, res=None, sample=None, overflow=None, unused=None,
                 scratch=None, plants=True, reads=None):
        self.n, self.tensors, self.batched, self.x, self.outs, self.launch, self.ref = n, tensors, batched, x, outs, launch, ref
        self.nonzero, self.res, self.sample = nonzero, res, tuple(sample) if sample is not None else tuple(range(n))
        self.overflow, self.unused, self.scratch, self.plants = overflow, unused or {}, scratch, plants
        self.reads = reads or (lambda r, c: True)


# ---- metro_conv_f16 / metro_conv_f32m / metro_conv_f64acc on a MetroConvDesc -------------------------------------------
def _big_pixel(d):
    """An input pixel some output reads through the centre tap (a strided or shifted layer does not read every pixel)."""
    ho, wo = d.h_out // 2, d.w_out // 2
    r = ho * d.stride - d.pad_top + (d.kh // 2) * d.dilation
    c = wo * d.stride - d.pad_left + (d.kw // 2) * d.dilation
    return int(np.clip(r, 0, d.h_in - 1)), int(np.clip(c, 0, d.w_in - 1))


def _reads(d):
    """(row, column) -> whether some tap of some output of `d` reads that input pixel (a strided or shifted layer skips some)."""
    def axis(size, n_out, k, pad):
        hit = np.zeros(size, bool)
        for o in range(n_out):
            for i in range(k):
                p = o * d.stride - pad + i * d.dilation
                if 0 <= p < size:
                    hit[p] = True
        return hit
    rows, cols = axis(d.h_in, d.h_out, d.kh, d.pad_top), axis(d.w_in, d.w_out, d.kw, d.pad_left)
    return lambda r, c: bool(rows[r] and cols[c])


def _overflow_pokes(xname, wname, sample, pixel, x_ch, w_ch, plus, minus):
    """Input channel x_ch of `pixel` becomes BIG_X in the first and the last reference image (different images: no output sees
    both); on that input channel, every tap of output channel `plus` weighs BIG_W and of `minus` -BIG_W."""
    pokes = [(xname, (img,) + pixel + (x_ch,), BIG_X) for img in sorted({sample[0], sample[-1]})]
    return pokes + [(wname, (plus, Ellipsis, w_ch), BIG_W), (wname, (minus, Ellipsis, w_ch), -BIG_W)]


def _desc_problem(case, d, kernel):
    """kernel: 'f16' (fp16 operands), 'f32m' (all fp32), 'f64acc' (fp32 activations, fp64 parameters)."""
    xdt, pdt, bdt = {'f16': (f16, f16, f32), 'f32m': (f32, f32, f32), 'f64acc': (f32, f64, f64)}[kernel]
    rng = _rng(kernel, case.name)
    x, w, b, pro, res = CC._operands(case, d, rng)
    off = case.off
    x = x.astype(xdt)
    used = np.zeros(d.in_pix_stride, bool)
    used[off:off + d.c_in] = True
    x[..., ~used] = 0
    t = {'x': x, 'w': _nz(w.astype(pdt)), 'b': _nz(b.astype(bdt))}
    if pro is not None:
        t['sc'], t['sh'] = pro[0].astype(pdt), _nz(pro[1].astype(pdt))
    if res is not None:
        t['res'] = res.astype(xdt)
    odt = {F16: f16, F32: f32, F64: f64}[d.out_dtype]
    fn = {'f16': 'metro_conv_f16', 'f32m': 'metro_conv_f32m', 'f64acc': 'metro_conv_f64acc'}[kernel]

    def launch(lib, p, o, scratch):
        px = C.c_void_p(p['x'].value + off * x.itemsize)
        check(getattr(lib, fn)(C.byref(d), px, p['w'], p['b'], _ptr(p, 'sc'), _ptr(p, 'sh'), _ptr(p, 'res'), o[0], None), f'{fn} {case.name}')

    def ref(t):
        ds = copy.copy(d)
        ds.n = t['x'].shape[0]
        xs = t['x'][..., off:off + d.c_in]
        pr = (t['sc'], t['sh']) if 'sc' in t else None
        k = d.kh * d.kw * d.c_in + 1
        if kernel != 'f16':          # relu, then the shortcut, in the accumulator's precision; one rounding to the output type
            y, _ = H.ref_conv_desc(ds, xs, t['w'], t['b'], pro=pr, pro_round=f32 if kernel == 'f32m' else None, res=t.get('res'))
            if kernel == 'f32m':     # tests/test_gpu_kernels.py:test_conv_f32m
                return [_out(_r(y, f32), y, rel=2e-5)], []
            return [_out(_r(y, f32), y, bound=0.5001 * H.ulp32(np.where(np.isfinite(y), y, 0.0)) + 1e-12)], []      # test_conv_f64acc
        dn = copy.copy(ds)
        dn.has_residual = 0
        y, a = H.ref_conv_desc(dn, xs, t['w'], t['b'], pro=pr)
        stages, rabs = [y], 0.0
        if d.out_dtype == F32:
            stored, rnd, floor = _r(y, f32), 2.0 ** -23, 2.0 ** -124
        else:
            stored, rnd, floor = _r(y, f16), 2.0 ** -10, 2.0 ** -24
            if 'res' in t:           # fp16(conv + bias), then the fp16 Add of the gathered shortcut
                rr = np.arange(d.h_out) * d.res_stride + d.res_offset
                rc = np.arange(d.w_out) * d.res_stride + d.res_offset
                rg = t['res'].astype(f64)[:, rr][:, :, rc]
                stages.append(stored + rg)
                stored, y, a, rabs = _r(stored + rg, f16), y + rg, a + np.abs(rg), np.abs(rg)
        # the per-element bound of tests/test_gpu_conv_contract.py; an element whose terms are not finite but which is itself
        # finite is a relu(-Inf): exactly zero, held to the floor
        fin = lambda v: np.where(np.isfinite(v), v, 0.0)
        bound = rnd * np.abs(fin(y)) + CC.C_SUM * 2.0 ** -24 * k * fin(a) + floor + rnd / 2 * fin(rabs)
        return [_out(stored, y, bound=bound)], stages

    overflow = None
    if kernel == 'f16' and d.out_dtype == F16:
        overflow = _overflow_pokes('x', 'w', case.sample or tuple(range(d.n)), _big_pixel(d), off + d.c_in // 2, d.c_in // 2, 1, d.c_out // 2 + 1)
    resinfo = ('res', d.res_stride, d.res_offset, d.h_out, d.w_out) if res is not None else None
    return Problem(d.n, t, {'x', 'res'}, ('x', off, d.c_in), [((d.n, d.h_out, d.w_out, d.c_out), odt)], launch, ref,
                   [k for k in t if k not in ('x', 'res')], res=resinfo, sample=case.sample, overflow=overflow,
                   unused={'x': ~used} if not used.all() else None, reads=_reads(d))


def _build_conv_f16(case):
    return _desc_problem(case, case.desc(), 'f16')


def _precise_case(name, variant):
    """A CONV_CASES row of tests/test_gpu_kernels.py as a contract Case (square maps, TF pads as the row states them)."""
    row = next(c for c in CONV_CASES if c[0] == name)
    _, n, h_in, c_in, c_out, k, stride, dil, pad, h_out = row
    assert variant != 'prologue' or (k == 1 and pad <= 0)
    return CC.Case(f'{name}-{variant}', '', n, h_in, h_in, c_in, c_out, k, k, stride, dil, pads=(pad, pad), relu=variant == 'relu_residual',
                   pro=variant == 'prologue', res=(1, 0) if variant == 'relu_residual' else None)


def _build_precise(kernel):
    def build(arg):
        case = _precise_case(*arg)
        d = case.desc(in_dtype=F32, out=F32)
        assert (d.h_out, d.w_out) == (next(c for c in CONV_CASES if c[0] == arg[0])[9],) * 2
        return _desc_problem(case, d, kernel)
    return build


# ---- the fused entry points -----------------------------------------------------------------------------------------------
def _second_gemm(out_stored, t):
    """conv1 of the next unit on the stored sum: relu(W2 . fp16(relu(out * scale2 + shift2)) + bias2), rounded once."""
    v = np.maximum(_mm(_pre(out_stored, t['sc2'], t['sh2']), t['w2'], t['b2']), 0.0)
    return v, _out(_r(v, f16), v)


def _next_params(rng, c1, c2):
    sc2, sh2 = _pro(rng, c1)
    return {'w2': _he(rng, c2, c1).reshape(c2, c1), 'b2': (rng.standard_normal(c2) * 0.1).astype(f32), 'sc2': sc2, 'sh2': sh2}


def _build_pair(shape):
    n, h, c_in, c_sc, cb = shape
    rng = _rng('pair', shape)
    sc, sh = _pro(rng, c_in)
    t = {'x': rng.standard_normal((n, h, h, c_in)).astype(f16), 'w': _he(rng, c_sc + cb, c_in), 'b': (rng.standard_normal(c_sc + cb) * 0.1).astype(f32),
         'sc': sc, 'sh': sh}
    d = H.conv_desc(n, h, c_in, h, c_sc + cb, 1, prologue=True, in_dtype=F16)

    def launch(lib, p, o, scratch):
        check(lib.metro_conv_f16_pair(C.byref(d), p['x'], p['w'], p['b'], p['sc'], p['sh'], o[0], c_sc, o[1], None), 'metro_conv_f16_pair')

    def ref(t):
        y = _mm(_pre(t['x'], t['sc'], t['sh']), t['w'], t['b'])
        y1, y2 = y[..., :c_sc], np.maximum(y[..., c_sc:], 0.0)
        return [_out(_r(y1, f16), y1), _out(_r(y2, f16), y2)], [y1, y2]

    pokes = _overflow_pokes('x', 'w', range(n), (h // 2, h // 2), c_in // 2, c_in // 2, 1, c_sc // 2 + 1)
    pokes.append(('w', (c_sc + cb - 2, Ellipsis, c_in // 2), BIG_W))          # and one channel of conv1's rows (behind their ReLU)
    return Problem(n, t, {'x'}, ('x', 0, c_in), [((n, h, h, c_sc), f16), ((n, h, h, cb), f16)], launch, ref, ['w', 'b', 'sc', 'sh'],
                   overflow=pokes)


def _build_next(shape):
    n, h = shape[:2]
    c_in = shape[2] if len(shape) > 2 else 64
    c1, c2 = 4 * c_in, c_in
    rng = _rng('next', shape)
    t = {'x': rng.standard_normal((n, h, h, c_in)).astype(f16), 'w': _he(rng, c1, c_in), 'b': (rng.standard_normal(c1) * 0.1).astype(f32),
         'res': rng.standard_normal((n, h, h, c1)).astype(f16), **_next_params(rng, c1, c2)}
    d = H.conv_desc(n, h, c_in, h, c1, 1, residual=True, res_h=h, in_dtype=F16)

    def launch(lib, p, o, scratch):
        check(lib.metro_conv_f16_next(C.byref(d), p['x'], p['w'], p['b'], p['res'], o[0], p['w2'], p['b2'], p['sc2'], p['sh2'], o[1], c2, None),
              'metro_conv_f16_next')

    def ref(t):
        conv = _mm(t['x'], t['w'], t['b'])
        s = _r(conv, f16) + t['res'].astype(f64)                          # fp16(conv3 + bias), then the fp16 Add
        v2, o2 = _second_gemm(_r(s, f16), t)
        return [_out(_r(s, f16), conv + t['res'].astype(f64)), o2], [conv, s, v2]

    return Problem(n, t, {'x', 'res'}, ('x', 0, c_in), [((n, h, h, c1), f16), ((n, h, h, c2), f16)], launch, ref,
                   ['w', 'b', 'w2', 'b2', 'sc2', 'sh2'], res=('res', 1, 0, h, h),
                   overflow=_overflow_pokes('x', 'w', range(n), (h // 2, h // 2), c_in // 2, c_in // 2, 1, c1 // 2 + 1))


def _build_conv1_conv2(shape):
    n, h = shape
    rng = _rng('c1c2', shape)
    ps, pb = _pro(rng, 64)
    t = {'x': rng.standard_normal((n, h, h, 64)).astype(f16), 'w1': _he(rng, 64, 64).reshape(64, 64),
         'b1': (rng.standard_normal(64) * 0.3 + 0.2).astype(f32), 'ps': ps, 'pb': pb, 'w2': _he(rng, 64, 64, 3),
         'b2': (rng.standard_normal(64) * 0.1).astype(f32)}
    d = H.conv_desc(n, h, 64, h, 64, 3, 1, 1, 1, relu=True, in_dtype=F16)

    def launch(lib, p, o, scratch):
        check(lib.metro_conv_f16_conv1_conv2(C.byref(d), p['x'], p['w1'], p['b1'], p['ps'], p['pb'], p['w2'], p['b2'], o[0], None),
              'metro_conv_f16_conv1_conv2')

    def ref(t):
        v1 = np.maximum(_mm(_pre(t['x'], t['ps'], t['pb']), t['w1'], t['b1']), 0.0)      # t1 lives in LDS as fp16: one rounding
        ds = copy.copy(d)
        ds.n = t['x'].shape[0]
        y, _ = H.ref_conv_desc(ds, _r(v1, f16), t['w2'], t['b2'])          # taps outside the image read zeros of t1 (d.relu = 1)
        return [_out(_r(y, f16), y)], [v1, y]

    # one pixel per image: the 3x3 windows of two +Inf of t1 would overlap into Inf - Inf
    return Problem(n, t, {'x'}, ('x', 0, 64), [((n, h, h, 64), f16)], launch, ref, ['w1', 'b1', 'ps', 'pb', 'w2', 'b2'],
                   overflow=_overflow_pokes('x', 'w1', range(n), (h // 2, h // 2), 32, 32, 1, 33))


def _proj_tensors(rng, n, h):
    ps, pb = _pro(rng, 64)
    return {'x': rng.standard_normal((n, h, h, 64)).astype(f16), 'w': _he(rng, 256, 64), 'b': (rng.standard_normal(256) * 0.1).astype(f32),
            'xu': rng.standard_normal((n, h, h, 64)).astype(f16), 'wsc': _he(rng, 256, 64).reshape(256, 64),
            'bsc': (rng.standard_normal(256) * 0.1).astype(f32), 'ps': ps, 'pb': pb}


def _proj_shortcut(t):
    v = _mm(_pre(t['xu'], t['ps'], t['pb']), t['wsc'], t['bsc'])
    return v, _r(v, f16)


def _build_next_proj(arg):
    n, h, store = arg                   # store = 0: the sum stays on chip (d_out NULL), the form metro_forward runs for block1/unit_1
    rng = _rng('nextproj', arg)
    t = {**_proj_tensors(rng, n, h), **_next_params(rng, 256, 64)}
    d = H.conv_desc(n, h, 64, h, 256, 1, in_dtype=F16)
    outs = ([((n, h, h, 256), f16)] if store else []) + [((n, h, h, 64), f16)]

    def launch(lib, p, o, scratch):
        check(lib.metro_conv_f16_next_proj(C.byref(d), p['x'], p['w'], p['b'], p['xu'], p['wsc'], p['bsc'], p['ps'], p['pb'],
                                           o[0] if store else None, p['w2'], p['b2'], p['sc2'], p['sh2'], o[-1], 64, None),
              'metro_conv_f16_next_proj')

    def ref(t):
        conv = _mm(t['x'], t['w'], t['b'])
        vsc, sc = _proj_shortcut(t)
        s = _r(conv, f16) + sc                                            # one rounding per addend, then the fp16 Add
        v2, o2 = _second_gemm(_r(s, f16), t)
        return ([_out(_r(s, f16), conv + vsc)] if store else []) + [o2], [conv, vsc, s, v2]

    return Problem(n, t, {'x', 'xu'}, ('x', 0, 64), outs, launch, ref, ['w', 'b', 'wsc', 'bsc', 'ps', 'pb', 'w2', 'b2', 'sc2', 'sh2'],
                   res=('xu', 1, 0, h, h), overflow=_overflow_pokes('x', 'w', range(n), (h // 2, h // 2), 32, 32, 1, 129))


def _build_next_rebuild(arg):
    n, h = arg                          # block1/unit_2 of a 256-pixel crop: tests/test_kernel_coverage.py:_conv
    rng = _rng('rebuild', arg)
    t = {**_proj_tensors(rng, n, h), 'tp': np.maximum(rng.standard_normal((n, h, h, 64)), 0).astype(f16),
         'w3p': _he(rng, 256, 64).reshape(256, 64), 'b3p': (rng.standard_normal(256) * 0.1).astype(f32), **_next_params(rng, 256, 64)}
    d = H.conv_desc(n, h, 64, h, 256, 1, in_dtype=F16)

    def launch(lib, p, o, scratch):
        check(lib.metro_conv_f16_next_rebuild(C.byref(d), p['x'], p['w'], p['b'], p['xu'], p['wsc'], p['bsc'], p['ps'], p['pb'], p['tp'],
                                              p['w3p'], p['b3p'], o[0], None, 0, p['w2'], p['b2'], p['sc2'], p['sh2'], o[1], 64, None),
              'metro_conv_f16_next_rebuild')

    def ref(t):
        vp = _mm(t['tp'], t['w3p'], t['b3p'])
        vsc, sc = _proj_shortcut(t)
        x1 = _r(vp, f16) + sc                                             # unit 1's sum, rebuilt: fp16(fp16 + fp16)
        conv = _mm(t['x'], t['w'], t['b'])
        s = _r(conv, f16) + _r(x1, f16)
        v2, o2 = _second_gemm(_r(s, f16), t)
        return [_out(_r(s, f16), conv + vp + vsc), o2], [vp, vsc, x1, conv, s, v2]

    return Problem(n, t, {'x', 'xu', 'tp'}, ('x', 0, 64), [((n, h, h, 256), f16), ((n, h, h, 64), f16)], launch, ref,
                   ['w', 'b', 'wsc', 'bsc', 'ps', 'pb', 'w3p', 'b3p', 'w2', 'b2', 'sc2', 'sh2'], res=('xu', 1, 0, h, h),
                   overflow=_overflow_pokes('x', 'w', range(n), (h // 2, h // 2), 32, 32, 1, 129))


def _build_gemm(arg):
    """A G8_CASES row of tests/test_gpu_kernels.py through conv_gemm4w (the product's kernel) or one of the experimental forms of
    libmetro_experimental.so, which metro_forward never dispatches but which share metro::relu."""
    kernel, name = arg
    _, n, c_in, c_out, variant = next(c for c in G8_CASES if c[0] == name)
    rng = _rng('gemm4w', name)           # the same operands for every kernel
    t = {'x': rng.standard_normal((n, 16, 16, c_in)).astype(f16), 'w': _he(rng, c_out, c_in).reshape(c_out, c_in),
         'b': (rng.standard_normal(c_out) * 0.1).astype(f32)}
    if 'prologue' in variant or variant == 'pair':
        t['sc'], t['sh'] = _pro(rng, c_in)
    if variant == 'residual':
        t['res'] = rng.standard_normal((n, 16, 16, c_out)).astype(f16)
    relu = 'relu' in variant
    split = c_out - 256 if variant == 'pair' else 0
    d = H.conv_desc(n, 16, c_in, 16, c_out, 1, prologue='sc' in t, relu=relu, residual='res' in t, res_h=16)
    outs = [((n, 16, 16, split or c_out), f16)] + ([((n, 16, 16, 256), f16)] if split else [])

    def launch(lib, p, o, scratch):
        entry = getattr(lib if kernel == 'gemm4w' else _lib.load_experimental(), f'metro_conv_f16_{kernel}')
        check(entry(C.byref(d), p['x'], p['w'], p['b'], _ptr(p, 'sc'), _ptr(p, 'sh'), _ptr(p, 'res'), o[0], split,
                    o[1] if split else None, None), f'metro_conv_f16_{kernel}')

    def ref(t):
        y = _mm(_pre(t['x'], t['sc'], t['sh']) if 'sc' in t else t['x'], t['w'], t['b'])
        if split:
            y1, y2 = y[..., :split], np.maximum(y[..., split:], 0.0)
            return [_out(_r(y1, f16), y1), _out(_r(y2, f16), y2)], [y1, y2]
        y = np.maximum(y, 0.0) if relu else y
        if 'res' in t:
            s = _r(y, f16) + t['res'].astype(f64)
            return [_out(_r(s, f16), y + t['res'].astype(f64))], [y, s]
        return [_out(_r(y, f16), y)], [y]

    pokes = _overflow_pokes('x', 'w', range(n), (8, 8), c_in // 2, c_in // 2, 1, (split or c_out) // 2 + 1)
    if split:
        pokes.append(('w', (c_out - 2, Ellipsis, c_in // 2), BIG_W))
    return Problem(n, t, {'x', 'res'}, ('x', 0, c_in), outs, launch, ref, [k for k in t if k not in ('x', 'res')],
                   res=('res', 1, 0, 16, 16) if 'res' in t else None, overflow=pokes)


# ---- the head: logits and poses -------------------------------------------------------------------------------------------
def _head_tensors(rng, spec, n, k=2048):
    side, c = spec.heatmap_side, spec.n_head_channels
    sc, sh = _pro(rng, k)
    return {'x': rng.standard_normal((n, side, side, k)).astype(f16), 'w': _he(rng, c, k, gain=2.0).reshape(c, k),
            'b': (rng.standard_normal(c) * 0.1).astype(f32), 'sc': sc, 'sh': sh}


def _head_ref(spec):
    from oracle.forward import logits_to_output

    def ref(t):
        y = _mm(_pre(t['x'], t['sc'], t['sh']), t['w'], t['b'])
        lg = _r(y, f32)
        poses = logits_to_output(H.oracle_spec(spec), y).numpy()          # the exact soft-argmax of the exact logits
        # tests/test_kernel_coverage.py:_head: logits 2e-5 of their maximum, poses 2e-3 mm
        return [_out(lg, y, rel=2e-5), _out(_r(poses, f32), poses, bound=np.full(poses.shape, 2e-3))], []
    return ref


def _build_head(arg):
    spec, n, k = arg if len(arg) == 3 else arg + (2048,)       # c_in: 2048 runs the ring kernel, 320 the plain 64- / 256-pixel ones
    side, c = spec.heatmap_side, spec.n_head_channels
    t = _head_tensors(_rng('head', spec, n, k), spec, n, k)
    cs = spec.to_c(_lib.METRO_PREC_F16)

    def launch(lib, p, o, scratch):
        check(lib.metro_head_f16(p['x'], p['w'], p['b'], p['sc'], p['sh'], n, k, C.byref(cs), scratch, o[0], o[1], None), 'metro_head_f16')

    return Problem(n, t, {'x'}, ('x', 0, k), [((n, side, side, c), f32), ((n, spec.skeleton.n_out, 3), f32)], launch, _head_ref(spec),
                   ['w', 'b', 'sc', 'sh'], scratch=lambda lib: lib.metro_head_f16_scratch_bytes(n, side, spec.skeleton.n_head),
                   sample=None if n <= 4 else (0, n - 1))


def _build_head_two_launch(arg):
    """A head that is not whole 64-pixel tiles: the fp32-output GEMM of metro_conv_f16, then metro_softargmax on its logits."""
    spec, n = arg
    side, k, c = spec.heatmap_side, 2048, spec.n_head_channels
    t = _head_tensors(_rng('head2', spec, n), spec, n)
    t['w'] = t['w'].reshape(c, 1, 1, k)
    cs = spec.to_c(_lib.METRO_PREC_F16)
    d = H.conv_desc(n, side, k, side, c, 1, prologue=True, out_dtype=F32, in_dtype=F16)

    def launch(lib, p, o, scratch):
        check(lib.metro_conv_f16(C.byref(d), p['x'], p['w'], p['b'], p['sc'], p['sh'], None, o[0], None), 'metro_conv_f16 (logits)')
        check(lib.metro_softargmax(o[0], n, C.byref(cs), _lib.METRO_PREC_F16, scratch, o[1], None), 'metro_softargmax')

    return Problem(n, t, {'x'}, ('x', 0, k), [((n, side, side, c), f32), ((n, spec.skeleton.n_out, 3), f32)], launch, _head_ref(spec),
                   ['w', 'b', 'sc', 'sh'], scratch=lambda lib: lib.metro_softargmax_scratch_bytes(n, side, spec.skeleton.n_head))


# ---- the stem: store overflow only ----------------------------------------------------------------------------------------
def _build_stem(arg):
    n, side = arg
    rng = _rng('stem', arg)
    w = (rng.standard_normal((64, 7, 7, 3)) * np.sqrt(2.0 / 147)).astype(f16)
    wp = np.zeros((64, 7, 8, 4), f16)                                    # [o][kh][kw + 1][c + 1]: the packed layout's zero tap and channel
    wp[:, :, :7, :3] = w
    t = {'img': rng.uniform(0, 1, (n, side, side, 3)).astype(f32), 'wp': wp, 'b': _nz((rng.standard_normal(64) * 0.5).astype(f32))}

    def launch(lib, p, o, scratch):
        check(lib.metro_stem_pool_f32in(p['img'], p['wp'], p['b'], o[0], n, side, None), 'metro_stem_pool_f32in')

    def ref(t):
        F = torch.nn.functional
        xi = torch.from_numpy(t['img'].astype(f16).astype(f64)).permute(0, 3, 1, 2)
        wt = torch.from_numpy(t['wp'][:, :, :7, :3].astype(f64)).permute(0, 3, 1, 2)
        conv = F.conv2d(F.pad(xi, (3, 3, 3, 3)), wt, torch.from_numpy(t['b'].astype(f64)), stride=2)
        pooled = F.max_pool2d(F.pad(conv.half().double(), (1, 1, 1, 1)), 3, 2).permute(0, 2, 3, 1).numpy()       # zero-padded pool
        return [_out(pooled, pooled)], [conv.numpy()]

    # a pixel of 2.5 in channel 1 under centre-tap weights of +-60000 (150 000 >= 2 * 65504); that channel of every other pixel is
    # halved (<= 30 000 <= 0.5 * 65504), which an image in [0, 0.5] is free to be
    t['img'][..., 1] *= 0.5
    pokes = [('img', (i, side // 2, side // 2 + 2 * i, 1), 2.5) for i in range(n)]
    pokes += [('wp', (1, 3, 3, 1), 60000.0), ('wp', (33, 3, 3, 1), -60000.0)]
    pr = Problem(n, t, {'img'}, ('img', 0, 3), [((n, side // 4, side // 4, 64), f16)], launch, ref, ['b'], overflow=pokes, plants=False)
    pr.nonzero_arrays = [w]
    return pr


_BUILDERS = {'conv_f16': _build_conv_f16, 'conv_f32m': _build_precise('f32m'), 'conv_f64acc': _build_precise('f64acc'),
             'pair': _build_pair, 'next': _build_next, 'conv1_conv2': _build_conv1_conv2, 'next_proj': _build_next_proj,
             'next_rebuild': _build_next_rebuild, 'gemm': _build_gemm, 'head': _build_head, 'head_two_launch': _build_head_two_launch,
             'stem': _build_stem}

_PRECISE_ROWS = [('3x3_s1', 'plain'), ('1x1_cin_tail', 'relu_residual'), ('1x1_ragged_m', 'prologue')]
_PRECISE_IDS = ['>', '>+res', ',pro>']            # how the ids of the three rows end
_FIN = 'softargmax_finalize<acc32>'

NF_CASES = [NFCase(c.name, (c.family,), 'conv_f16', c) for c in CC.CASES] + \
    [NFCase('-'.join(r), ('conv_igemm_f32<64x128,bk32,v4' + x,), 'conv_f32m', r) for r, x in zip(_PRECISE_ROWS, _PRECISE_IDS)] + \
    [NFCase('-'.join(r), ('conv_igemm_f64acc<in32,act32,128x64,v2' + x,), 'conv_f64acc', r) for r, x in zip(_PRECISE_ROWS, _PRECISE_IDS)] + [
    NFCase('block1_ragged', ('conv_pw64<k64,wm4,pro,pair>',), 'pair', (3, 7, 64, 256, 64)),
    NFCase('block2', ('conv_pw64<k256,wm8,cb512,pro,pair>',), 'pair', (2, 16, 256, 512, 128)),
    NFCase('ragged', ('conv_pw64<k64,wm4,res,next>',), 'next', (3, 7)),
    NFCase('block2_small', ('conv_pw64<k128,wm8,cb512,res,next>',), 'next', (2, 8, 128)),
    NFCase('one_image', ('conv3x3_c64<pre1>',), 'conv1_conv2', (1, 64)),
    NFCase('16map', ('conv3x3_c64<pre1>',), 'conv1_conv2', (9, 16)),
    NFCase('ragged', ('conv_pw64<k64,wm4,next,projsc>',), 'next_proj', (3, 7, 1)),
    # the producer / consumer kernel of conv_b1.hip, at the shape of its first layer in tests/test_kernel_coverage.py:CONFIGS (C1)
    NFCase('on_chip_64map', ('conv_b1_chain<projsc,noout>',), 'next_proj', (1, 64, 0)),
    NFCase('64map', ('conv_b1_chain<rebuild>',), 'next_rebuild', (1, 64)),
    NFCase('k128', ('conv_gemm4w<256x256>',), 'gemm', ('gemm4w', 'k128')),                 # the smallest whole-tile case of G8_CASES ...
    NFCase('k256_relu', ('conv_gemm4w<256x256>',), 'gemm', ('gemm4w', 'k256_relu')),       # ... and its ReLU epilogue, its prologue, its pair routing
    NFCase('k512_pro', ('conv_gemm4w<256x256,pro>',), 'gemm', ('gemm4w', 'k512_pro')),
    NFCase('pair_k256', ('conv_gemm4w<256x256,pro>+pair',), 'gemm', ('gemm4w', 'pair_k256')),
    NFCase('rn50-s32-h36m-n3', ('head_f16<144x64,k4>', _FIN), 'head', (ModelSpec(50, 32, 'h36m'), 3)),
    NFCase('rn50-s16-many19-n2', ('head_f16<160x64,k4>', _FIN), 'head', (ModelSpec(50, 16, 'many19'), 2)),
    # three joint groups: the 424-channel head, on the 16 x 16 heat map of a 64-pixel crop
    NFCase('rn50-s4-merged53-side64-n1', ('head_f16<160x64,k4,g3>', _FIN), 'head', (ModelSpec(50, 4, 'merged', proc_side=64), 1)),
    NFCase('rn50-s32-h36m-side224-n2', ('conv_igemm_f16_dma<64x128,bk64,s3,pro>+f32out', 'softargmax_partial<acc32,logits32>', _FIN), 'head_two_launch',
           (ModelSpec(50, 32, 'h36m', proc_side=224), 2)),
    # the two kernels of head_f16.hip that are not the ring kernel (c_in 320 is not ring-eligible), at the shapes of
    # tests/test_gpu_heat_moments.py:HEAD_CASES: 64-pixel tiles, and the 256-pixel tiles of a launch of >= 256 tiles
    NFCase('plain64-n1', ('head_f16<160x64>', _FIN), 'head', (ModelSpec(50, 16, 'h36m'), 1, 320)),
    NFCase('plain256-n16', ('head_f16<160x256>', _FIN), 'head', (ModelSpec(50, 4, 'h36m'), 16, 320)),
    NFCase('2x64', ('stem_pool_f16<split2,f32in>',), 'stem', (2, 64)),
    NFCase('1x256', ('stem_pool_f16<rows,f32in>',), 'stem', (1, 256)),
] + [NFCase(f'{k}-{nm}', (f'conv_{k}<256x256{x}>',), 'gemm', (k, nm))       # libmetro_experimental.so: the ReLU epilogue, the prologue
     for k in ('gemm8p', 'gemm4d') for nm, x in (('k256_relu', ''), ('k512_pro', ',pro'))]


def dry_run_ids(lib, case):
    """The kernel ids the case's launches would note (metro_kernel_notes(2): nothing is launched, no device is needed)."""
    pr = case.problem()
    p = {name: _DRY for name in pr.tensors}
    check(lib.metro_kernel_notes(2), 'metro_kernel_notes')
    try:
        pr.launch(lib, p, [_DRY] * len(pr.outs), _DRY)
        return lib.metro_last_kernel_id().decode().split(' & ')
    finally:
        lib.metro_kernel_notes(0)


def ids_match(ids, families):
    """A family that is a whole id ('...>' with whatever follows it) must be the id; the conv-contract table's own entries, which
    end inside the brackets, are prefixes."""
    return len(ids) == len(families) and all(k == f if '>' in f else k.startswith(f) for k, f in zip(ids, families))


def kernel_of(kid):
    """The __global__ kernel behind an id: its family (the text in front of '<'), and, where one family holds several kernels
    with a ReLU or a store of their own, which of them (head_f16.hip: ring / 256-pixel / plain; stem_pool_f16.hip: rows / patch)."""
    fam = kid.split('<')[0]
    if fam == 'head_f16':
        return fam + (':ring' if ',k' in kid else ':256' if 'x256' in kid else ':plain')
    if fam == 'stem_pool_f16':
        return fam + (':rows' if '<rows' in kid else ':patch')
    return fam


# ---- the allocation, the plants, the comparison -----------------------------------------------------------------------------
class Arena:
    """Every input of a launch in one allocation: BAND | tensor (padded to 256 bytes) | BAND, one after the other."""

    def __init__(self, pr):
        self.pr, self.off, self.span, pos = pr, {}, {}, 0
        for name, a in pr.tensors.items():
            padded = -(-a.nbytes // 256) * 256
            self.off[name], self.span[name] = pos + BAND, (pos, pos + BAND + padded + BAND)
            pos += BAND + padded + BAND
        self.size = pos

    def host(self, poison):
        """The allocation's bytes: bands, padding and the unused elements inside a tensor hold NaN of the tensor's type
        (`poison`) or zeros."""
        buf = np.zeros(self.size, np.uint8)
        for name, a in self.pr.tensors.items():
            lo, hi = self.span[name]
            if poison:
                buf[lo:hi].view(UINT[a.itemsize])[:] = NAN_BITS[a.itemsize]
            data = a.copy()
            if name in self.pr.unused:
                data[np.broadcast_to(self.pr.unused[name], data.shape)] = np.nan if poison else 0.0
            buf[self.off[name]:self.off[name] + a.nbytes] = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        return buf

    def view(self, buf, name):
        a = self.pr.tensors[name]
        return buf[self.off[name]:self.off[name] + a.nbytes].view(TORCH[a.dtype]).view(a.shape)

    def ptrs(self, buf):
        return {name: C.c_void_p(buf.data_ptr() + off) for name, off in self.off.items()}


def plants(pr):
    """[(tensor, index, value)]: the three special values at the three positions of the input, and at one element of the residual."""
    if not pr.plants:
        return []
    name, off, c_in = pr.x
    n, h, w, _ = pr.tensors[name].shape
    tile = 256 if h * w >= 256 else 64
    g = tile - 1 if tile - 1 < n * h * w else n * h * w // 2
    img, pix = divmod(g, h * w)
    if img not in pr.sample:
        img, pix = pr.sample[0], min(tile - 1, h * w - 1)
    while not pr.reads(pix // w, pix % w) and pix + 1 < h * w:       # a strided or shifted layer skips pixels: the next one it reads
        pix += 1
    spots = [(name, (0, 0, 0, off)), (name, (n - 1, h - 1, w - 1, off + c_in - 1)), (name, (img, pix // w, pix % w, off + c_in // 2))]
    if pr.res is not None:           # the residual element the first output pixel behind the tile boundary reads
        rname, rs, ro, ho, wo = pr.res
        ri, rp = divmod(min(tile, n * ho * wo - 1), ho * wo)
        if ri not in pr.sample:
            ri, rp = pr.sample[-1], min(tile, ho * wo - 1)
        spots.append((rname, (ri, rp // wo * rs + ro, rp % wo * rs + ro, pr.tensors[rname].shape[-1] // 2)))
    return [(nm, idx, v) for v in SPECIALS for nm, idx in spots]


def pack(pl):
    """Launches of at most one plant per image."""
    launches = []
    for p in pl:
        for group in launches:
            if all(q[1][0] != p[1][0] for q in group):
                group.append(p)
                break
        else:
            launches.append([p])
    return launches


def classes(a):
    """0 finite, 1 +Inf, 2 -Inf, 3 NaN."""
    a = np.asarray(a, f64)
    return np.isposinf(a) * 1 + np.isneginf(a) * 2 + np.isnan(a) * 3


def _bits(a):
    return np.ascontiguousarray(a).view(UINT[a.itemsize])


_CLASS_NAMES = ('finite', '+Inf', '-Inf', 'NaN')


def compare(case, pr, got, clean, ref, ref0, what, params_changed=False):
    """The three assertions of the module docstring on every output; returns whether the plant influenced any element.
    params_changed: the plant is also in the weights, so images outside the reference's sample are not those of the clean launch."""
    sample, influenced = list(pr.sample), False
    others = [i for i in range(pr.n) if i not in pr.sample]
    for k, (g_all, c_all, r, r0) in enumerate(zip(got, clean, ref, ref0)):
        tag = f'{case.id} ({"/".join(sorted(case.family_names()))}) {what}, output {k}'
        g, c = g_all[sample], c_all[sample]
        g64 = g.astype(f64)
        gc, rc = classes(g64), classes(r.stored)
        if not (gc == rc).all():
            at = tuple(int(v) for v in np.argwhere(gc != rc)[0])
            raise AssertionError(f'{tag}: {int((gc != rc).sum())} of {gc.size} elements are not of the reference\'s class; first at {at} '
                                 f'(reference image {sample[at[0]]}): got {g64[at]!r} ({_CLASS_NAMES[gc[at]]}), the reference has '
                                 f'{r.stored[at]!r} ({_CLASS_NAMES[rc[at]]})')
        same = (r.exact == r0.exact) & np.isfinite(r.stored) & np.isfinite(r0.stored)     # the fp64 values: a term that moves only below the store's rounding is still a term
        moved = same & (_bits(g) != _bits(c))
        assert not moved.any(), f'{tag}: {int(moved.sum())} elements the plant cannot reach differ from the clean launch; first at {np.argwhere(moved)[0]}'
        if others and not params_changed:
            assert np.array_equal(_bits(g_all[others]), _bits(c_all[others])), f'{tag}: an image without a plant differs from the clean launch'
        infl = ~same & np.isfinite(r.stored)
        with np.errstate(invalid='ignore'):
            err = np.abs(g64 - r.exact)
            out = infl & ~(err <= r.bound)
        assert not out.any(), (f'{tag}: {int(out.sum())} influenced finite elements out of bound; first at {np.argwhere(out)[0]}: '
                               f'got {g64[out][0]!r} want {r.exact[out][0]!r} bound {r.bound[out][0]:.3g}')
        influenced |= bool((~same).any())
    return influenced


def _poked(pr, ts, pokes):
    """The reference's tensors (batched ones restricted to pr.sample) with `pokes` applied; pokes in other images are dropped."""
    t = dict(ts)
    for name, idx, v in pokes:
        if name in pr.batched:
            if idx[0] not in pr.sample:
                continue
            idx = (pr.sample.index(idx[0]),) + tuple(idx[1:])
        if t[name] is ts[name]:
            t[name] = ts[name].copy()
        t[name][idx] = v
    return t


def _launch(lib, cuda, pr, arena, base, pokes):
    buf = base.clone() if pokes else base
    for name, idx, v in pokes:
        arena.view(buf, name)[idx] = v
    outs = [torch.full(shape, float('nan'), dtype=TORCH[np.dtype(dt)], device=cuda) for shape, dt in pr.outs]
    scratch = torch.empty(int(pr.scratch(lib)), dtype=torch.uint8, device=cuda) if pr.scratch else None
    pr.launch(lib, arena.ptrs(buf), [H.ptr(o) for o in outs], H.ptr(scratch))
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize('case', NF_CASES, ids=[c.id for c in NF_CASES])
def test_special_values_through_one_kernel(lib, cuda, case):
    pr = case.problem()
    for a in getattr(pr, 'nonzero_arrays', []) + [pr.tensors[k] for k in pr.nonzero]:
        assert np.isfinite(a).all() and (a != 0).all(), f'{case.id}: a zero (or non-finite) parameter'
    arena = Arena(pr)
    zeros = torch.from_numpy(arena.host(False)).to(cuda)
    check(lib.metro_kernel_notes(1), 'metro_kernel_notes')
    try:
        clean = _launch(lib, cuda, pr, arena, zeros, [])
        ids = lib.metro_last_kernel_id().decode().split(' & ')
    finally:
        lib.metro_kernel_notes(0)
    assert ids_match(ids, case.families), f'{case.id}: launched {ids}, meant for {case.families}'
    ts = {name: (a[list(pr.sample)] if name in pr.batched else a) for name, a in pr.tensors.items()}
    with np.errstate(all='ignore'):
        ref0, _ = pr.ref(ts)
    for r in ref0:
        assert np.isfinite(r.stored).all(), f'{case.id}: the clean reference is not finite'
    # clean: every element counts as influenced -- finite and within the bound of the case's existing test
    hollow = [SimpleNamespace(stored=np.full(r.stored.shape, np.nan), exact=r.exact, bound=r.bound) for r in ref0]
    compare(case, pr, clean, clean, ref0, hollow, 'clean')

    influenced = not pr.plants
    for group in pack(plants(pr)):
        got = _launch(lib, cuda, pr, arena, zeros, group)
        with np.errstate(all='ignore'):
            ref, _ = pr.ref(_poked(pr, ts, group))
        what = ' + '.join(f'{v} at {name}{list(idx)}' for name, idx, v in group)
        influenced |= compare(case, pr, got, clean, ref, ref0, what)
    assert influenced, f'{case.id}: no plant reached any output'

    if pr.overflow is not None:
        got = _launch(lib, cuda, pr, arena, zeros, pr.overflow)
        with np.errstate(all='ignore'):
            ref, stages = pr.ref(_poked(pr, ts, pr.overflow))
        for s in stages:             # the gap: a condition on the inputs (module docstring, 4.)
            mag = np.abs(s)
            assert ((mag >= 2 * F16_MAX) | (mag <= 0.5 * F16_MAX)).all(), f'{case.id}: the overflow plant leaves values near the fp16 maximum'
        assert any(np.isinf(r.stored).any() for r in ref), f'{case.id}: the overflow plant overflows nothing'
        compare(case, pr, got, clean, ref, ref0, 'store overflow from finite data', params_changed=True)

    nans = torch.from_numpy(arena.host(True)).to(cuda)
    poisoned = _launch(lib, cuda, pr, arena, nans, [])
    for k, (g, c) in enumerate(zip(poisoned, clean)):
        assert np.array_equal(_bits(g), _bits(c)), \
            (f'{case.id} ({"/".join(sorted(case.family_names()))}), output {k}: NaN around the inputs (or in the unused channels of a '
             f'pixel) changes {int((_bits(g) != _bits(c)).sum())} elements: the launch uses what it reads outside its tensors')
