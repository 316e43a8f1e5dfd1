"""The epilogue stores of every conv family through the C ABI (`-m gpu`): what a launch writes, where, and what the next
launch on the stream reads of it.

A kernel file chooses the form of its 16-byte activation stores (metro_common.h: store_out16 -- plain, or write-through,
which leaves nothing dirty in the L2 when the launch ends).  The form may change neither a byte nor an address, and what a
launch stored must be what its consumer reads, without any host synchronisation in between.  Every case runs one launch of a
family at the smallest shape its *_supported predicate admits -- a few tiles, one to four images, with a ragged or predicated
last tile where the family has one -- and checks, for the output and for the second or sub-sampled output where there is one:

  1. the values, against the fp64 restatement and the bound of the family's existing test (the problems and references are
     those of tests/test_gpu_nonfinite_kernels.py; the conv-contract rows carry the per-element bound of
     tests/test_gpu_conv_contract.py, the fused launches 2e-3 of the layer maximum);
  2. that every element was written (the outputs start as NaN) and that the 4 KiB guard bands in front of and behind each
     output still hold their sentinel;
  3. that a second launch on the same stream, issued right behind the first with no synchronisation, reads of each output
     the very bits a host copy reads afterwards.

What this file is and is not.  The store form is a property of the build, and no case looks at kernel code: every check holds
for the plain form as for the write-through one, so the file states the contract a store form must keep -- values, addresses,
every element written -- on each epilogue path, ragged and predicated ones included; it does not tell the forms apart and
does not guard the write-through path as such.  Check 3 in particular passes for any store that has reached memory or the L2
by the end of its kernel, which the launch boundary guarantees for both forms: it would catch a store lost or torn, not a form."""
import copy
import ctypes as C
from dataclasses import dataclass

import numpy as np
import pytest
import torch

from metro_pose3d_amd import _lib
from metro_pose3d_amd._lib import check
from tests import helpers as H
from tests import test_gpu_conv_contract as CC
from tests import test_gpu_nonfinite_kernels as NF

pytestmark = pytest.mark.gpu

F16 = _lib.METRO_F16
f16, f32, f64 = np.float16, np.float32, np.float64
XOR = {torch.float16: (torch.int16, 0x5555), torch.float32: (torch.int32, 0x55555555)}


# ---- two launches the borrowed builders do not state -----------------------------------------------------------------------
def _build_next_plain(shape):
    """metro_conv_f16_next without a residual: conv3 + the next unit's conv1 on the ring kernel's two-GEMM form."""
    n, h = shape
    c_in, c1, c2 = 64, 256, 64
    rng = NF._rng('store_forms/next_plain', shape)
    t = {'x': rng.standard_normal((n, h, h, c_in)).astype(f16), 'w': NF._he(rng, c1, c_in),
         'b': (rng.standard_normal(c1) * 0.1).astype(f32), **NF._next_params(rng, c1, c2)}
    d = H.conv_desc(n, h, c_in, h, c1, 1, in_dtype=F16)

    def launch(lib, p, o, scratch):
        check(lib.metro_conv_f16_next(C.byref(d), p['x'], p['w'], p['b'], None, o[0], p['w2'], p['b2'], p['sc2'], p['sh2'], o[1], c2, None),
              'metro_conv_f16_next (no residual)')

    def ref(t):
        conv = NF._mm(t['x'], t['w'], t['b'])
        v2, o2 = NF._second_gemm(NF._r(conv, f16), t)
        return [NF._out(NF._r(conv, f16), conv), o2], [conv, v2]

    return NF.Problem(n, t, {'x'}, ('x', 0, c_in), [((n, h, h, c1), f16), ((n, h, h, c2), f16)], launch, ref,
                      ['w', 'b', 'w2', 'b2', 'sc2', 'sh2'])


def _build_next_rebuild_sub(arg):
    """metro_conv_f16_next_rebuild storing only the pixels (sub_off + 2 i, sub_off + 2 j) of its sum, on the producer / consumer
    kernel (classic = 0) or the single-role kernel of conv_pw64.hip (classic = 1)."""
    n, h, sub_off, classic = arg
    pr = NF._build_next_rebuild((n, h))
    full_ref = pr.ref
    hs = (h - sub_off + 1) // 2
    d = H.conv_desc(n, h, 64, h, 256, 1, in_dtype=F16)

    def launch(lib, p, o, scratch):
        check(lib.metro_conv_b1_form(classic), 'metro_conv_b1_form')
        try:
            check(lib.metro_conv_f16_next_rebuild(C.byref(d), p['x'], p['w'], p['b'], p['xu'], p['wsc'], p['bsc'], p['ps'], p['pb'], p['tp'],
                                                  p['w3p'], p['b3p'], None, o[0], sub_off, p['w2'], p['b2'], p['sc2'], p['sh2'], o[1], 64, None),
                  'metro_conv_f16_next_rebuild (sub-sampled sum)')
        finally:
            lib.metro_conv_b1_form(0)

    def ref(t):
        (s, o2), stages = full_ref(t)
        cut = lambda a: np.ascontiguousarray(a[:, sub_off::2, sub_off::2])
        return [NF._out(cut(s.stored), cut(s.exact), bound=cut(s.bound)), o2], stages

    pr.launch, pr.ref = launch, ref
    pr.outs = [((n, hs, hs, 256), f16), ((n, h, h, 64), f16)]
    return pr


def _classic(build):
    """The builder's launch with the test switch on: conv_pw64.hip's kernel where conv_b1.hip's or conv_pws.hip's is the default."""
    def wrapped(arg):
        pr = build(arg)
        inner = pr.launch

        def launch(lib, p, o, scratch):
            check(lib.metro_conv_b1_form(1), 'metro_conv_b1_form')
            try:
                inner(lib, p, o, scratch)
            finally:
                lib.metro_conv_b1_form(0)
        pr.launch = launch
        return pr
    return wrapped


@dataclass
class StoreCase:
    name: str
    families: tuple             # the launches' kernel ids, in order (NF.ids_match)
    build: object
    arg: object

    @property
    def id(self):
        return self.name


def _row(name):
    case = next(c for c in CC.CASES if c.name == name)
    return StoreCase(name, (case.family,), NF._build_conv_f16, case)


B = NF._BUILDERS
CASES = [
    # ---- stem_pool_f16.hip: the patch kernel and the rows kernel
    StoreCase('stem_2x64', ('stem_pool_f16<split2,f32in>',), B['stem'], (2, 64)),
    StoreCase('stem_1x256', ('stem_pool_f16<rows,f32in>',), B['stem'], (1, 256)),
    # ---- conv3x3_c64.hip: plain, and with conv1 in front (9 images of 16 x 16: more tiles than one round of blocks holds evenly)
    _row('c64_4x64'),
    _row('c64_16x8'),
    StoreCase('c64_pre1_16map', ('conv3x3_c64<pre1>',), B['conv1_conv2'], (9, 16)),
    # ---- conv_b1.hip: the whole sum, and its sub-sampled pixels at both offsets
    StoreCase('b1_rebuild', ('conv_b1_chain<rebuild>',), B['next_rebuild'], (2, 16)),
    StoreCase('b1_rebuild_sub0', ('conv_b1_chain<rebuild,subout>',), _build_next_rebuild_sub, (2, 16, 0, 0)),
    StoreCase('b1_rebuild_sub1', ('conv_b1_chain<rebuild,subout>',), _build_next_rebuild_sub, (2, 16, 1, 0)),
    # ---- conv_pw64.hip: 147 pixels (a ragged last tile) in the pair, next and projection-shortcut forms; the residual gather;
    #      the 512-channel rows of block2; the sub-sampled sum of the single-role kernel
    StoreCase('pw64_pair_ragged', ('conv_pw64<k64,wm4,pro,pair>',), B['pair'], (3, 7, 64, 256, 64)),
    StoreCase('pw64_next_ragged', ('conv_pw64<k64,wm4,res,next>',), B['next'], (3, 7)),
    StoreCase('pw64_next_proj_ragged', ('conv_pw64<k64,wm4,next,projsc>',), B['next_proj'], (3, 7, 1)),
    StoreCase('pw64_next_block2', ('conv_pw64<k128,wm8,cb512,res,next>',), B['next'], (2, 8, 128)),
    _row('pw64_7x13_res_sub'),
    _row('pw128_6x10_res'),
    StoreCase('pw64_rebuild_sub1_classic', ('conv_pw64<k64,wm4,next,projsc,rebuild,subout>',), _build_next_rebuild_sub, (2, 16, 1, 1)),
    # ---- conv_pws.hip (192 pixels: one and a half tiles) and the kernel it replaces, on the same rows
    _row('pws_8x12_res'),
    StoreCase('pws_8x12_res_classic', (CC.PW64,), _classic(NF._build_conv_f16), next(c for c in CC.CASES if c.name == 'pws_8x12_res')),
    # ---- conv3x3_f16_slab.hip: 384 pixels, and rows that cross images
    _row('c64_4x32_m384'),
    _row('slab_12x32_cross_images'),
    # ---- conv_igemm_f16_dma.hip: ragged pixel tiles, a channel tail (the scalar stores behind the 16-byte ones), fp32 rows,
    #      the pair routing and the two-GEMM form
    _row('dma_7x13'),
    _row('cout132_f16'),
    _row('cout12_f32'),
    _row('res_rect_s2_off1'),
    StoreCase('dma_pair_256_72', ('conv_igemm_f16_dma<128x128,bk64,s1,pro>+pair',), B['pair'], (2, 16, 64, 256, 72)),
    StoreCase('dma_fuse2', ('conv_igemm_f16_fuse2<256x64>',), _build_next_plain, (2, 16)),
    StoreCase('dma_fuse2_ragged', ('conv_igemm_f16_fuse2<256x64>',), _build_next_plain, (3, 7)),
    # ---- conv_gemm4w.hip (whole 256-pixel tiles only): plain and pair routing
    StoreCase('g4_k128', ('conv_gemm4w<256x256>',), B['gemm'], ('gemm4w', 'k128')),
    StoreCase('g4_pair_k256', ('conv_gemm4w<256x256,pro>+pair',), B['gemm'], ('gemm4w', 'pair_k256')),
]


@pytest.mark.parametrize('case', CASES, ids=[c.id for c in CASES])
def test_stores_land_whole_in_place_and_visible_to_the_next_launch(lib, cuda, case):
    pr = case.build(case.arg)
    arena = NF.Arena(pr)
    base = torch.from_numpy(arena.host(False)).to(cuda)
    guarded = [CC._guarded(shape, NF.TORCH[np.dtype(dt)], cuda) for shape, dt in pr.outs]
    outs = [g[0] for g in guarded]
    scratch = torch.empty(int(pr.scratch(lib)), dtype=torch.uint8, device=cuda) if pr.scratch else None
    torch.cuda.synchronize()
    check(lib.metro_kernel_notes(1), 'metro_kernel_notes')
    try:
        pr.launch(lib, arena.ptrs(base), [H.ptr(o) for o in outs], H.ptr(scratch))
        # the consumer: one elementwise launch per output on the same stream, nothing in between
        seen = [torch.bitwise_xor(o.view(XOR[o.dtype][0]), XOR[o.dtype][1]) for o in outs]
        torch.cuda.synchronize()
        ids = lib.metro_last_kernel_id().decode().split(' & ')
    finally:
        lib.metro_kernel_notes(0)
    assert NF.ids_match(ids, case.families), f'{case.id}: launched {ids}, meant for {case.families}'
    for k, (_, buf) in enumerate(guarded):
        assert CC._guards_intact(buf), f'{case.id} ({ids}), output {k}: a store landed outside the tensor'
    host = [o.cpu().numpy() for o in outs]
    for k, (s, g, o) in enumerate(zip(seen, host, outs)):
        want = NF._bits(g) ^ NF.UINT[g.itemsize](XOR[o.dtype][1])
        got = NF._bits(s.cpu().numpy())
        assert np.array_equal(got, want), (f'{case.id} ({ids}), output {k}: the next launch on the stream read {int((got != want).sum())} '
                                           f'of {got.size} elements other than the host copy holds')
    ts = {name: (a[list(pr.sample)] if name in pr.batched else a) for name, a in pr.tensors.items()}
    with np.errstate(all='ignore'):
        ref, _ = pr.ref(ts)
    for k, (g, r) in enumerate(zip(host, ref)):
        assert np.isfinite(g).all(), f'{case.id} ({ids}), output {k}: {int((~np.isfinite(g)).sum())} elements not written (or not finite)'
        err = np.abs(g[list(pr.sample)].astype(f64) - r.exact)
        bad = ~(err <= r.bound)
        assert not bad.any(), (f'{case.id} ({ids}), output {k}: {int(bad.sum())} of {bad.size} elements out of bound; worst '
                               f'{float((err / np.maximum(r.bound, 1e-300)).max()):.3g} x the bound')
