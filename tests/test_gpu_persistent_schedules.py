"""Every persistent conv kernel on every tile-walk schedule (`-m gpu`; the classifier and the case table are checked on the CPU).

Five launchers cap their grid at CUs x resident blocks per CU (metro_common.h: ensure_dyn_lds_and_grid_cap) and let a block walk
several tiles: conv_pw64, conv_pws, conv_b1_chain, conv3x3_c64 and stem_pool_f16<split*>.  Inside their tile loops correctness
depends on how many tiles a block has already run and on what the previous tile did: the buffer `it & 1` and the counted
`wait_vm` of conv_pw64 (which counts the stores the PREVIOUS tile left in flight, so it changes with prev_full and prev_sub),
the three-slot ring and the ramp / drain of conv_pws and conv_b1_chain (T = tiles of this block), the two slabs of conv3x3_c64
with its clipped last block, the three windows of the stem.  The shape-level tests reach some of these states by accident; here
each is a named class, and every instantiation is launched once on each class its predicate admits.

The grid cap is known on the device only.  metro_last_launch_schedule (include/metro_hip.h) reports what the launcher used:
(grid, work items, cap, halves).  A first one-tile launch of an instantiation yields its cap C; G = C / halves is the number of
tile streams of a capped grid, and the classes are tile counts in terms of G:

    class         tiles        what it reaches
    plain-map     7            grid below the cap and not a multiple of 8: the fallback block map, one tile per stream
    xcd-map       8            grid below the cap, the XCD-grouped block map, one tile per stream
    cap           G            every stream exactly one tile at the capped grid
    cap+1         G + 1        one stream runs 2 tiles while the others drain after 1
    two           2 G          every stream uses both buffers and ends on buffer 1
    two-three     2 G + G/2    2 and 3 tiles per stream in one launch: streams end on either buffer
    long          5 G - 1      4 and 5 tiles per stream: the steady state
    ragged-late   2 G + 1      the last tile holds TN - 5 pixels and is the THIRD tile of stream 0 (where the predicate admits a
                               ragged pixel count: the conv_pw64 forms that do not need whole 64-pixel maps)

conv_b1_chain has no block map (block b starts at tile b), so `plain-map` and `xcd-map` are one class there, `below-cap` (7 tiles).
The stem has none either and its classes are named by patches per block: `ppb1-below` (7 patches), `ppb1` (G), `ppb1-2` (G + 1),
`ppb2` (2 G), `ppb2-3` (2 G + G/2), `ppb4-5` (5 G - 1).  conv3x3_c64 gives a block `tiles_per_block` CONSECUTIVE tiles: its classes
are tiles_per_block 1, 2 and 3, the last two with a short last block.

The sub-sampled-output forms run `two-three` four times, on 16-wide and on 64-wide maps, each with sub_off 0 and 1.  conv_pw64's
counted wait takes the number of sub-sampled stores the PREVIOUS tile of the stream issued (prev_sub).  On the 4 x 16 maps a tile
is a whole image and every tile issues two of its four row-wise instructions: prev_sub is constant.  On the 64-wide maps a tile
is one map row, kept whole or not at all.  A stream walks tiles t, t + G, t + 2 G, so with TWO rows per image and an even G every
tile of a stream would be the same row; the maps are 3 x 64 (three tiles per image, the tile count rounded up to whole images):
with G = 256 a stream sees rows r, r + 1, r + 2 mod 3, which is all / none / all at sub_off 0 and none / all / none at 1.  Each
case ASSERTS this from the recorded grid and work (sub_store_transitions): on the 64-wide maps some stream goes from a tile with
all four stores to one with none and some stream the other way; on the 16-wide maps the count never changes.  A cap that is a
multiple of three would fail that assertion rather than quietly run another class.

Shapes are the smallest the predicates admit: one tile per image (8 x 8 maps for 64-pixel tiles, 4 x 8 for 32-pixel ones, 4 x 16
where the width must be a power of two >= 16, 8 x 16 for conv3x3_c64, 32 x 32 crops for the stem), so the image count is the tile
count; the 64-wide maps are 3 x 64; ragged-late is one image of 1 x m pixels.

Every case launches ONCE and asserts
  * the kernel id (metro_last_kernel_id) is the instantiation it names;
  * the recorded schedule classifies (schedule_class) as the class it names: a changed cap or grid rule cannot quietly move a
    case onto another class;
  * the outputs start as NaN between 4 KiB guard bands: every element is written, the guards are intact;
  * the values agree with the fp64 restatement of the same fp16 operands under the bound the family already has: the per-element
    bound of tests/test_gpu_conv_contract.py for the plain launches (metro_conv_f16), 2e-3 of the layer maximum for the fused
    launches and the stem (tests/test_gpu_nonfinite_kernels.py).  No new tolerance.
The reference covers every pixel where it forms at most REF_MACS multiply-adds and REF_ELEMS elements (Inst.macs, Inst.elems per
pixel; calls of up to four images always).  The limits come from the heaviest plain case, conv_pws K = 512 -> 2048 on 5 G - 1 =
159 tiles: 5 088 pixels, 1.07e10 multiply-adds (the product and the condition sum |x| |w| of the per-element bound are one
matmul each) and 3.1e7 elements, measured at 0.3 - 1.3 s of numpy on eight cores, and from 1.3e8 elements of a 64 -> 256 layer
at 1.2 s: REF_MACS = 1.2e10, REF_ELEMS = 4e7 keep a case's reference under about a second.  Anything larger is built from four
base images laid out with tests/helpers.py: crop_assignment; positions 0..3 are held to fp64 and every other position to its
twin's bits (assert_twins): with one-tile images that is every tile of every stream.

Measured on an MI355X (256 CUs), as the cases print it (`-s`).  Grid cap C:

    512   conv_pw64<k64,wm4,pro> and the three stem_pool_f16<split2*> (two resident blocks per CU)
    256   every other instantiation (one block per CU): the other fourteen conv_pw64 forms, both conv_pws, the three
          conv_b1_chain, conv3x3_c64 with and without conv1 in front

so G = C / halves is 512 (k64 pro, the stems), 256 (halves 1), 128 (conv_pw64 k128 wm4: 2 halves), 64 (k256 wm8 and conv_pws k256:
4 halves) and 32 (k512: 8 halves), and the tile counts per class follow from the table: at G = 256 they are 7, 8, 256, 257, 512,
640, 1279 and 513 (ragged-late: 32 827 pixels), and 642 tiles = 214 images on the 3 x 64 maps, where prev_sub -> now_sub takes
(4, 0), (0, 4) and (4, 4) at sub_off 0 and (0, 4), (4, 0) and (0, 0) at sub_off 1; at G = 32 they are 7, 8, 32, 33, 64, 80, 159 and
65; conv3x3_c64 runs 256, 257 and 514 tiles.  All 180 cases passed once, 28 s in all (the slowest 0.9 s); 127 of them hold every
pixel to fp64, 53 four base images and their twins.  Worst error as a share of the bound: conv_pw64 0.90 (k64 res; the fused
forms 0.32), conv_pws 0.67, conv_b1_chain 0.34, conv3x3_c64 0.24, the stem 0.29.
"""
import ctypes as C
from collections import namedtuple
from dataclasses import dataclass, field

import numpy as np
import pytest
import torch

from metro_pose3d_amd import _lib
from metro_pose3d_amd._lib import check
from tests import helpers as H
from tests import test_gpu_conv_contract as CC
from tests import test_gpu_nonfinite_kernels as NF

F16 = _lib.METRO_F16
f16, f32, f64 = np.float16, np.float32, np.float64
REF_MACS, REF_ELEMS = 1.2e10, 4e7      # a reference of every pixel: at most this many fp64 multiply-adds and elements (module docstring)
BASE_IMAGES = 4


# ---- the classifier --------------------------------------------------------------------------------------------------------
Schedule = namedtuple('Schedule', 'streams t_min t_max n_max branch')


def schedule_class(grid, work, cap, halves, walk='strided'):
    """What a launch with this record does: the tile streams G, the fewest and the most tiles a stream runs, how many streams
    run the most, and the block map's branch ('xcd' | 'plain', as metro_common.h: block_stream_map decides it).
    walk 'strided': stream s runs tiles s, s + G, ... (conv_pw64, conv_pws, conv_b1_chain, the stem); 'contiguous': block b runs
    tiles [b tpb, (b + 1) tpb) with tpb = ceil(work / cap) (conv3x3_c64; cap > 0)."""
    assert grid > 0 and halves > 0 and grid % halves == 0 and work % halves == 0 and work >= grid
    streams, tiles = grid // halves, work // halves
    branch = 'xcd' if grid % 8 == 0 and (grid // 8) % halves == 0 else 'plain'
    if walk == 'contiguous':
        assert halves == 1 and cap > 0
        tpb = -(-work // cap)
        assert grid == -(-work // tpb)
        last = work - (grid - 1) * tpb                      # the clipped last block
        return Schedule(streams, last, tpb, grid - (last < tpb), branch)
    t_min, t_max = tiles // streams, -(-tiles // streams)
    return Schedule(streams, t_min, t_max, streams if t_min == t_max else tiles - t_min * streams, branch)


# the stem's classes, named by patches per block, and the tile-count class each one is
STEM_NAMES = {'ppb1-below': 'below-cap', 'ppb1': 'cap', 'ppb1-2': 'cap+1', 'ppb2': 'two', 'ppb2-3': 'two-three', 'ppb4-5': 'long'}
W64_ROWS = 3                    # rows of the 64-wide maps of the sub-sampled-output cases (module docstring: coprime to G)


def _base(cls):
    b = cls.split('/')[0]
    return STEM_NAMES.get(b, b)


def class_tiles(cls, g, cap=None):
    """Work items (pixel tiles, patches) of a class at G tile streams (cap: conv3x3_c64's classes)."""
    if '/w64' in cls:               # whole images of W64_ROWS one-row tiles
        return -(-(2 * g + g // 2) // W64_ROWS) * W64_ROWS
    if cls.startswith('tpb'):
        k = int(cls[3])
        t = (k - 1) * cap + 1 if k > 1 else cap
        while k > 1 and t % k == 0:
            t += 1
        return t
    return {'plain-map': 7, 'below-cap': 7, 'xcd-map': 8, 'cap': g, 'cap+1': g + 1, 'two': 2 * g, 'two-three': 2 * g + g // 2,
            'long': 5 * g - 1, 'ragged-late': 2 * g + 1}[_base(cls)]


def expected_schedule(cls, g, cap=None):
    """The Schedule fields a class stands for (None: not part of the class)."""
    base = _base(cls)
    if base.startswith('tpb'):
        k, t = int(base[3]), class_tiles(base, g, cap)
        return Schedule(-(-t // k), t - (-(-t // k) - 1) * k, k, None, None)
    return {'plain-map': Schedule(7, 1, 1, 7, 'plain'), 'below-cap': Schedule(7, 1, 1, 7, None), 'xcd-map': Schedule(8, 1, 1, 8, 'xcd'),
            'cap': Schedule(g, 1, 1, g, None), 'cap+1': Schedule(g, 1, 2, 1, None), 'two': Schedule(g, 2, 2, g, None),
            'two-three': Schedule(g, 2, 3, class_tiles(cls, g) - 2 * g, None), 'long': Schedule(g, 4, 5, g - 1, None),
            'ragged-late': Schedule(g, 2, 3, 1, None)}[base]


def sub_stores_of_tile(tile, h, w, sub_off, tn=64):
    """conv_pw64's OUTM = 2 epilogue (now_sub): how many of the tile's tn / 16 row-wise instructions hold pixels of map rows
    sub_off, sub_off + 2, ... -- instruction r covers pixels 16 r .. 16 r + 15 of the tile, one map row (w >= 16, a power of two)."""
    h_sub, rem0 = (h - sub_off + 1) // 2, tile * tn % (h * w)
    rows = [(rem0 + 16 * r) // w - sub_off for r in range(tn // 16)]
    return sum(1 for hr in rows if hr >= 0 and hr % 2 == 0 and hr // 2 < h_sub)


def sub_store_transitions(grid, work, h, w, sub_off):
    """{(stores of a tile, stores of the next tile of the same stream)} over every stream of a launch of `work` tiles on `grid`
    streams (halves 1): the values prev_sub -> now_sub takes."""
    return {(sub_stores_of_tile(t, h, w, sub_off), sub_stores_of_tile(t + grid, h, w, sub_off)) for t in range(work - grid)}


def matches(got, want):
    return all(w is None or v == w for v, w in zip(got, want))


def test_schedule_class_on_hand_computed_rows():
    # (grid, work, cap, halves) -> streams, t_min, t_max, streams that run t_max, branch
    rows = [((7, 7, 512, 1), (7, 1, 1, 7, 'plain')),
            ((8, 8, 512, 1), (8, 1, 1, 8, 'xcd')),
            ((512, 513, 512, 1), (512, 1, 2, 1, 'xcd')),
            ((512, 1280, 512, 1), (512, 2, 3, 256, 'xcd')),
            ((512, 2559, 512, 1), (512, 4, 5, 511, 'xcd')),
            ((28, 28, 256, 4), (7, 1, 1, 7, 'plain')),             # 7 tiles x 4 halves: 28 & 7 != 0
            ((56, 56, 256, 8), (7, 1, 1, 7, 'plain')),             # 56 & 7 == 0 but 56 / 8 = 7 is no multiple of 8 halves
            ((64, 64, 256, 8), (8, 1, 1, 8, 'xcd')),
            ((256, 264, 256, 8), (32, 1, 2, 1, 'xcd')),            # G = 32, 33 tiles
            ((256, 1272, 256, 8), (32, 4, 5, 31, 'xcd')),          # 159 tiles = 4 x 32 + 31
            ((256, 516, 256, 4), (64, 2, 3, 1, 'xcd')),            # 129 tiles: the third tile of stream 0
            ((252, 504, 254, 4), (63, 2, 2, 63, 'plain')),         # a cap of 254 (a partitioned device): grid 252, 252 & 7 = 4
            ((240, 240, 240, 2), (120, 1, 1, 120, 'xcd')),         # 240 / 8 = 30 is a multiple of 2 halves
            ((120, 120, 120, 2), (60, 1, 1, 60, 'plain'))]         # 120 / 8 = 15 is not
    for args, want in rows:
        assert tuple(schedule_class(*args)) == want, (args, tuple(schedule_class(*args)), want)
    # contiguous ranges (conv3x3_c64): cap 256
    assert tuple(schedule_class(256, 256, 256, 1, 'contiguous')) == (256, 1, 1, 256, 'xcd')
    assert tuple(schedule_class(129, 257, 256, 1, 'contiguous')) == (129, 1, 2, 128, 'plain')       # tpb 2, the last block holds 1
    assert tuple(schedule_class(172, 514, 256, 1, 'contiguous')) == (172, 1, 3, 171, 'plain')       # tpb 3, 171 x 3 + 1
    assert tuple(schedule_class(4, 4, 256, 1, 'contiguous')) == (4, 1, 1, 4, 'plain')
    # the classes' tile counts and what they stand for, at G = 64
    assert [class_tiles(c, 64) for c in STRIDED] == [7, 8, 64, 65, 128, 160, 319] and class_tiles('ragged-late', 64) == 129
    assert [class_tiles(c, None, 256) for c in C64_CLASSES] == [256, 257, 514]
    assert matches(schedule_class(256, 160 * 4, 256, 4), expected_schedule('two-three', 64))
    assert not matches(schedule_class(256, 161 * 4, 256, 4), expected_schedule('two-three', 64))
    assert not matches(schedule_class(256, 128 * 4, 256, 4), expected_schedule('ragged-late', 64))
    assert [class_tiles(c, 512) for c in STEM_CLASSES] == [7, 512, 513, 1024, 1280, 2559]
    assert expected_schedule('ppb2-3', 512) == expected_schedule('two-three', 512) == Schedule(512, 2, 3, 256, None)
    # the sub-sampled stores along a stream: 3 x 64 maps at G = 256 (642 tiles) alternate, 2 x 64 maps would not; 4 x 16 is constant
    assert class_tiles('two-three/w64-off0', 256) == 642 and expected_schedule('two-three/w64-off1', 256) == Schedule(256, 2, 3, 130, None)
    assert [sub_stores_of_tile(t, 3, 64, 0) for t in range(4)] == [4, 0, 4, 4] and [sub_stores_of_tile(t, 3, 64, 1) for t in range(4)] == [0, 4, 0, 0]
    assert sub_store_transitions(256, 642, 3, 64, 0) == {(4, 0), (0, 4), (4, 4)}
    assert sub_store_transitions(256, 642, 3, 64, 1) == {(0, 4), (4, 0), (0, 0)}
    assert sub_store_transitions(256, 640, 2, 64, 0) == {(4, 4), (0, 0)}            # two rows, even G: every stream keeps its row
    assert sub_store_transitions(258, 645, 3, 64, 0) == {(4, 4), (0, 0)}            # ... as do three rows at a G that 3 divides
    assert sub_store_transitions(256, 640, 4, 16, 0) == sub_store_transitions(256, 640, 4, 16, 1) == {(2, 2)}
    assert matches(schedule_class(172, 514, 256, 1, 'contiguous'), expected_schedule('tpb3-short', None, 256))
    assert not matches(schedule_class(171, 513, 256, 1, 'contiguous'), expected_schedule('tpb3-short', None, 256))


# ---- the problems: p base images of h x w pixels, a descriptor of n images -------------------------------------------------
@dataclass
class Prob:
    tensors: dict               # name -> numpy array (the batched ones hold p images)
    batched: set
    outs: list                  # per-image shapes of the outputs (fp16)
    launch: object              # (lib, q: name -> c_void_p, o: [c_void_p]) -> None
    ref: object                 # (tensors) -> [NF._out per output] for the p base images
    scratch: dict = field(default_factory=dict)     # name -> (per-image shape, torch dtype): device-only buffers of n images


def _rng(*parts):
    return NF._rng('schedules', *parts)


def _forced_classic(launch):
    def wrapped(lib, q, o):
        check(lib.metro_conv_b1_form(1), 'metro_conv_b1_form')
        try:
            launch(lib, q, o)
        finally:
            lib.metro_conv_b1_form(0)
    return wrapped


def _b_plain(c_in, c_out, pro=False, res=None, classic=False):
    """metro_conv_f16 on a 1x1 layer; res = (stride, offset) of the shortcut gather."""
    def build(n, p, h, w):
        rng = _rng('plain', c_in, c_out, pro, res, h, w)
        rs, ro = res or (1, 0)
        rh, rw = ((h - 1) * rs + ro + 1 + (ro > 0), (w - 1) * rs + ro + 1) if res else (0, 0)
        t = {'x': rng.standard_normal((p, h, w, c_in)).astype(f16), 'w': NF._he(rng, c_out, c_in),
             'b': (rng.standard_normal(c_out) * 0.1).astype(f32)}
        if pro:
            t['sc'], t['sh'] = NF._pro(rng, c_in)
        if res:
            t['res'] = rng.standard_normal((p, rh, rw, c_out)).astype(f16)
        d = H.conv_desc(n, h, c_in, h, c_out, 1, prologue=pro, residual=res is not None, res_h=rh, res_w=rw, res_stride=rs,
                        res_offset=ro, w_in=w, w_out=w, in_dtype=F16)

        def launch(lib, q, o):
            check(lib.metro_conv_f16(C.byref(d), q['x'], q['w'], q['b'], NF._ptr(q, 'sc'), NF._ptr(q, 'sh'), NF._ptr(q, 'res'), o[0], None),
                  'metro_conv_f16')

        def ref(t):
            x = NF._pre(t['x'], t['sc'], t['sh']) if pro else t['x'].astype(f64)
            wm, b = t['w'].astype(f64).reshape(c_out, c_in), t['b'].astype(f64)
            y, a = x @ wm.T + b, np.abs(x) @ np.abs(wm).T + np.abs(b)
            stored, rabs = NF._r(y, f16), 0.0
            if res:                  # fp16(conv + bias), then the fp16 Add of the gathered shortcut
                rg = t['res'].astype(f64)[:, ro::rs, ro::rs][:, :h, :w]
                stored, y, a, rabs = NF._r(stored + rg, f16), y + rg, a + np.abs(rg), np.abs(rg)
            # the per-element bound of tests/test_gpu_conv_contract.py (K = c_in products + the bias)
            bound = 2.0 ** -10 * np.abs(y) + CC.C_SUM * 2.0 ** -24 * (c_in + 1) * a + 2.0 ** -24 + 2.0 ** -11 * rabs
            return [NF._out(stored, y, bound=bound)]
        return Prob(t, {'x', 'res'}, [(h, w, c_out)], _forced_classic(launch) if classic else launch, ref)
    return build


def _b_pair(c_in, c_sc, cb):
    def build(n, p, h, w):
        rng = _rng('pair', c_in, h, w)
        sc, sh = NF._pro(rng, c_in)
        t = {'x': rng.standard_normal((p, h, w, c_in)).astype(f16), 'w': NF._he(rng, c_sc + cb, c_in),
             'b': (rng.standard_normal(c_sc + cb) * 0.1).astype(f32), 'sc': sc, 'sh': sh}
        d = H.conv_desc(n, h, c_in, h, c_sc + cb, 1, prologue=True, w_in=w, w_out=w, in_dtype=F16)

        def launch(lib, q, o):
            check(lib.metro_conv_f16_pair(C.byref(d), q['x'], q['w'], q['b'], q['sc'], q['sh'], o[0], c_sc, o[1], None), 'metro_conv_f16_pair')

        def ref(t):
            y = NF._mm(NF._pre(t['x'], t['sc'], t['sh']), t['w'], t['b'])
            y1, y2 = y[..., :c_sc], np.maximum(y[..., c_sc:], 0.0)
            return [NF._out(NF._r(y1, f16), y1), NF._out(NF._r(y2, f16), y2)]
        return Prob(t, {'x'}, [(h, w, c_sc), (h, w, cb)], launch, ref)
    return build


def _b_next(c_in):
    def build(n, p, h, w):
        c1, c2 = 4 * c_in, c_in
        rng = _rng('next', c_in, h, w)
        t = {'x': rng.standard_normal((p, h, w, c_in)).astype(f16), 'w': NF._he(rng, c1, c_in), 'b': (rng.standard_normal(c1) * 0.1).astype(f32),
             'res': rng.standard_normal((p, h, w, c1)).astype(f16), **NF._next_params(rng, c1, c2)}
        d = H.conv_desc(n, h, c_in, h, c1, 1, residual=True, res_h=h, res_w=w, w_in=w, w_out=w, in_dtype=F16)

        def launch(lib, q, o):
            check(lib.metro_conv_f16_next(C.byref(d), q['x'], q['w'], q['b'], q['res'], o[0], q['w2'], q['b2'], q['sc2'], q['sh2'], o[1], c2, None),
                  'metro_conv_f16_next')

        def ref(t):
            conv = NF._mm(t['x'], t['w'], t['b'])
            s = NF._r(conv, f16) + t['res'].astype(f64)
            _, o2 = NF._second_gemm(NF._r(s, f16), t)
            return [NF._out(NF._r(s, f16), conv + t['res'].astype(f64)), o2]
        return Prob(t, {'x', 'res'}, [(h, w, c1), (h, w, c2)], launch, ref)
    return build


def _proj_tensors(rng, p, h, w):
    ps, pb = NF._pro(rng, 64)
    return {'x': rng.standard_normal((p, h, w, 64)).astype(f16), 'w': NF._he(rng, 256, 64), 'b': (rng.standard_normal(256) * 0.1).astype(f32),
            'xu': rng.standard_normal((p, h, w, 64)).astype(f16), 'wsc': NF._he(rng, 256, 64).reshape(256, 64),
            'bsc': (rng.standard_normal(256) * 0.1).astype(f32), 'ps': ps, 'pb': pb}


def _b_next_proj(store):
    """store = 0: the sum stays on chip (d_out NULL)."""
    def build(n, p, h, w):
        rng = _rng('next_proj', store, h, w)
        t = {**_proj_tensors(rng, p, h, w), **NF._next_params(rng, 256, 64)}
        d = H.conv_desc(n, h, 64, h, 256, 1, w_in=w, w_out=w, in_dtype=F16)

        def launch(lib, q, o):
            check(lib.metro_conv_f16_next_proj(C.byref(d), q['x'], q['w'], q['b'], q['xu'], q['wsc'], q['bsc'], q['ps'], q['pb'],
                                               o[0] if store else None, q['w2'], q['b2'], q['sc2'], q['sh2'], o[-1], 64, None),
                  'metro_conv_f16_next_proj')

        def ref(t):
            conv = NF._mm(t['x'], t['w'], t['b'])
            vsc, sc = NF._proj_shortcut(t)
            s = NF._r(conv, f16) + sc
            _, o2 = NF._second_gemm(NF._r(s, f16), t)
            return ([NF._out(NF._r(s, f16), conv + vsc)] if store else []) + [o2]
        return Prob(t, {'x', 'xu'}, ([(h, w, 256)] if store else []) + [(h, w, 64)], launch, ref)
    return build


def _b_next_rebuild(sub, classic):
    """sub = False: the whole sum is stored; True: only its pixels (sub_off + 2 i, sub_off + 2 j) (build's keyword sub_off)."""
    def build(n, p, h, w, sub_off=0):
        rng = _rng('rebuild', h, w)
        t = {**_proj_tensors(rng, p, h, w), 'tp': np.maximum(rng.standard_normal((p, h, w, 64)), 0).astype(f16),
             'w3p': NF._he(rng, 256, 64).reshape(256, 64), 'b3p': (rng.standard_normal(256) * 0.1).astype(f32), **NF._next_params(rng, 256, 64)}
        d = H.conv_desc(n, h, 64, h, 256, 1, w_in=w, w_out=w, in_dtype=F16)
        hs, ws = (h - sub_off + 1) // 2, (w - sub_off + 1) // 2

        def launch(lib, q, o):
            check(lib.metro_conv_f16_next_rebuild(C.byref(d), q['x'], q['w'], q['b'], q['xu'], q['wsc'], q['bsc'], q['ps'], q['pb'], q['tp'],
                                                  q['w3p'], q['b3p'], None if sub else o[0], o[0] if sub else None, sub_off, q['w2'], q['b2'],
                                                  q['sc2'], q['sh2'], o[1], 64, None), 'metro_conv_f16_next_rebuild')

        def ref(t):
            vp = NF._mm(t['tp'], t['w3p'], t['b3p'])
            vsc, sc = NF._proj_shortcut(t)
            x1 = NF._r(vp, f16) + sc
            conv = NF._mm(t['x'], t['w'], t['b'])
            s = NF._r(conv, f16) + NF._r(x1, f16)
            _, o2 = NF._second_gemm(NF._r(s, f16), t)
            full = NF._out(NF._r(s, f16), conv + vp + vsc)
            if sub:
                cut = lambda a: np.ascontiguousarray(a[:, sub_off::2, sub_off::2])
                full = NF._out(cut(full.stored), cut(full.exact), bound=cut(full.bound))
            return [full, o2]
        return Prob(t, {'x', 'xu', 'tp'}, [(hs, ws, 256) if sub else (h, w, 256), (h, w, 64)], _forced_classic(launch) if classic else launch, ref)
    return build


def _b_c64(pre1):
    def build(n, p, h, w):
        import copy
        rng = _rng('c64', pre1, h, w)
        t = {'x': rng.standard_normal((p, h, w, 64)).astype(f16), 'w2': NF._he(rng, 64, 64, 3), 'b2': (rng.standard_normal(64) * 0.1).astype(f32)}
        if pre1:
            ps, pb = NF._pro(rng, 64)
            t.update({'w1': NF._he(rng, 64, 64).reshape(64, 64), 'b1': (rng.standard_normal(64) * 0.3 + 0.2).astype(f32), 'ps': ps, 'pb': pb})
        d = H.conv_desc(n, h, 64, h, 64, 3, 1, 1, 1, relu=True, w_in=w, w_out=w, in_dtype=F16)

        def launch(lib, q, o):
            if pre1:
                check(lib.metro_conv_f16_conv1_conv2(C.byref(d), q['x'], q['w1'], q['b1'], q['ps'], q['pb'], q['w2'], q['b2'], o[0], None),
                      'metro_conv_f16_conv1_conv2')
            else:
                check(lib.metro_conv_f16(C.byref(d), q['x'], q['w2'], q['b2'], None, None, None, o[0], None), 'metro_conv_f16')

        def ref(t):
            ds = copy.copy(d)
            ds.n = t['x'].shape[0]
            if pre1:                 # t1 lives in LDS as fp16: one rounding
                v1 = np.maximum(NF._mm(NF._pre(t['x'], t['ps'], t['pb']), t['w1'], t['b1']), 0.0)
                y, _ = H.ref_conv_desc(ds, NF._r(v1, f16), t['w2'], t['b2'])
                return [NF._out(NF._r(y, f16), y)]
            y, a = H.ref_conv_desc(ds, t['x'], t['w2'], t['b2'])
            return [NF._out(NF._r(y, f16), y, bound=2.0 ** -10 * np.abs(y) + CC.C_SUM * 2.0 ** -24 * 577 * a + 2.0 ** -24)]
        return Prob(t, {'x'}, [(h, w, 64)], launch, ref)
    return build


def _b_stem(kind):
    """kind: 'f32in' | 'u8in' | 'prepped' (metro_prep_input_f16 in front of metro_stem_pool_f16)."""
    def build(n, p, h, w):
        side = h
        rng = _rng('stem', kind, side)
        wk = (rng.standard_normal((64, 7, 7, 3)) * np.sqrt(2.0 / 147)).astype(f16)
        wp = np.zeros((64, 7, 8, 4), f16)
        wp[:, :, :7, :3] = wk
        img = rng.integers(0, 256, (p, side, side, 3), dtype=np.uint8) if kind == 'u8in' else rng.uniform(0, 1, (p, side, side, 3)).astype(f32)
        t = {'img': img, 'wp': wp, 'b': (rng.standard_normal(64) * 0.5).astype(f32)}

        def launch(lib, q, o):
            if kind == 'prepped':
                check(lib.metro_prep_input_f16(q['img'], n, side, q['prepped'], None), 'metro_prep_input_f16')
                check(lib.metro_stem_pool_f16(q['prepped'], q['wp'], q['b'], o[0], n, side, None), 'metro_stem_pool_f16')
            else:
                fn = lib.metro_stem_pool_u8in if kind == 'u8in' else lib.metro_stem_pool_f32in
                check(fn(q['img'], q['wp'], q['b'], o[0], n, side, None), f'metro_stem_pool_{kind}')

        def ref(t):
            F = torch.nn.functional
            im = t['img'].astype(f32) / f32(255) if kind == 'u8in' else t['img']
            xi = torch.from_numpy(im.astype(f16).astype(f64)).permute(0, 3, 1, 2)
            wt = torch.from_numpy(t['wp'][:, :, :7, :3].astype(f64)).permute(0, 3, 1, 2)
            conv = F.conv2d(F.pad(xi, (3, 3, 3, 3)), wt, torch.from_numpy(t['b'].astype(f64)), stride=2)
            pooled = F.max_pool2d(F.pad(conv.half().double(), (1, 1, 1, 1)), 3, 2).permute(0, 2, 3, 1).numpy()
            return [NF._out(pooled, pooled)]
        scratch = {'prepped': ((side + 6, side + 8, 4), torch.float16)} if kind == 'prepped' else {}
        return Prob(t, {'img'}, [(side // 4, side // 4, 64)], launch, ref, scratch)
    return build


# ---- the instantiations ------------------------------------------------------------------------------------------------------
@dataclass
class Inst:
    kid: str                    # the kernel id of the instantiation
    family: str                 # 'pw64' | 'pws' | 'b1' | 'c64' | 'stem'
    build: object
    tn: int                     # pixels of a tile (stem: the crop side of one patch)
    halves: int
    tile_map: tuple             # (h, w) of one work item
    ragged: bool = False        # the predicate admits a pixel count that is no multiple of tn
    macs: int = 0               # fp64 multiply-adds of the reference per pixel
    elems: int = 0              # elements the reference forms per pixel
    before: tuple = ()          # ids noted in front of the kernel's own

    @property
    def walk(self):
        return 'contiguous' if self.family == 'c64' else 'strided'

    @property
    def min_items(self):
        return 4 if self.family == 'c64' else 1        # conv3x3_c64: at least four 128-pixel tiles


B1_MAP = (4, 16)
INSTANCES = [
    # every launch_pw<...> launch_conv_pw64 reaches (conv_pw64.hip), in its order
    Inst('conv_pw64<k256,wm8,cb512,pro,pair>', 'pw64', _b_pair(256, 512, 128), 32, 1, (4, 8), True, 256 * 640, 640 * 2),
    Inst('conv_pw64<k64,wm4,pro,pair>', 'pw64', _b_pair(64, 256, 64), 64, 1, (8, 8), True, 64 * 320, 320 * 2),
    Inst('conv_pw64<k64,wm4,next,projsc,rebuild,subout>', 'pw64', _b_next_rebuild(True, True), 64, 1, B1_MAP, False, 64 * 768 + 256 * 64, 2000),
    Inst('conv_pw64<k64,wm4,next,projsc,rebuild>', 'pw64', _b_next_rebuild(False, True), 64, 1, B1_MAP, False, 64 * 768 + 256 * 64, 2000),
    Inst('conv_pw64<k64,wm4,next,projsc,noout>', 'pw64', _b_next_proj(0), 64, 1, (8, 8), True, 64 * 512 + 256 * 64, 1500),
    Inst('conv_pw64<k64,wm4,next,projsc>', 'pw64', _b_next_proj(1), 64, 1, (8, 8), True, 64 * 512 + 256 * 64, 1500),
    Inst('conv_pw64<k128,wm8,cb512,res,next>', 'pw64', _b_next(128), 32, 1, (4, 8), True, 128 * 512 + 512 * 128, 2500),
    Inst('conv_pw64<k64,wm4,res,next>', 'pw64', _b_next(64), 64, 1, (8, 8), True, 64 * 256 + 256 * 64, 1300),
    Inst('conv_pw64<k512,wm8,res>', 'pw64', _b_plain(512, 2048, res=(1, 0), classic=True), 32, 8, (4, 8), True, 2 * 512 * 2048, 2048 * 3),
    Inst('conv_pw64<k256,wm8,res>', 'pw64', _b_plain(256, 1024, res=(1, 0), classic=True), 32, 4, (4, 8), True, 2 * 256 * 1024, 1024 * 3),
    Inst('conv_pw64<k128,wm4,res,ressub>', 'pw64', _b_plain(128, 512, res=(2, 1)), 64, 2, (8, 8), True, 2 * 128 * 512, 512 * 3),
    Inst('conv_pw64<k128,wm4,res>', 'pw64', _b_plain(128, 512, res=(1, 0)), 64, 2, (8, 8), True, 2 * 128 * 512, 512 * 3),
    Inst('conv_pw64<k64,wm4,pro>', 'pw64', _b_plain(64, 256, pro=True), 64, 1, (8, 8), True, 2 * 64 * 256, 256 * 3),
    Inst('conv_pw64<k64,wm4,res,ressub>', 'pw64', _b_plain(64, 256, res=(2, 1)), 64, 1, (8, 8), True, 2 * 64 * 256, 256 * 3),
    Inst('conv_pw64<k64,wm4,res>', 'pw64', _b_plain(64, 256, res=(1, 0)), 64, 1, (8, 8), True, 2 * 64 * 256, 256 * 3),
    # conv_pws.hip: whole 32-pixel tiles only
    Inst('conv_pws<k256,res>', 'pws', _b_plain(256, 1024, res=(1, 0)), 32, 4, (4, 8), False, 2 * 256 * 1024, 1024 * 3),
    Inst('conv_pws<k512,res>', 'pws', _b_plain(512, 2048, res=(1, 0)), 32, 8, (4, 8), False, 2 * 512 * 2048, 2048 * 3),
    # conv_b1.hip: whole 64-pixel tiles of maps whose width is a power of two >= 16
    Inst('conv_b1_chain<projsc,noout>', 'b1', _b_next_proj(0), 64, 1, B1_MAP, False, 64 * 512 + 256 * 64, 1500),
    Inst('conv_b1_chain<rebuild>', 'b1', _b_next_rebuild(False, False), 64, 1, B1_MAP, False, 64 * 768 + 256 * 64, 2000),
    Inst('conv_b1_chain<rebuild,subout>', 'b1', _b_next_rebuild(True, False), 64, 1, B1_MAP, False, 64 * 768 + 256 * 64, 2000),
    # conv3x3_c64.hip: 128-pixel tiles of whole map rows
    Inst('conv3x3_c64', 'c64', _b_c64(False), 128, 1, (8, 16), False, 2 * 9 * 64 * 64, 64 * 12),
    Inst('conv3x3_c64<pre1>', 'c64', _b_c64(True), 128, 1, (8, 16), False, 10 * 64 * 64, 64 * 12),
    # stem_pool_f16.hip's patch kernel: one 8 x 8 pooled patch per 32 x 32 crop
    Inst('stem_pool_f16<split2,f32in>', 'stem', _b_stem('f32in'), 32, 1, (32, 32), False, 256 * 147 * 64 // 1024, 64),
    Inst('stem_pool_f16<split2,u8in>', 'stem', _b_stem('u8in'), 32, 1, (32, 32), False, 256 * 147 * 64 // 1024, 64),
    Inst('stem_pool_f16<split2>', 'stem', _b_stem('prepped'), 32, 1, (32, 32), False, 256 * 147 * 64 // 1024, 64, before=('prep_input_f16',)),
]
BY_ID = {i.kid: i for i in INSTANCES}

STRIDED = ('plain-map', 'xcd-map', 'cap', 'cap+1', 'two', 'two-three', 'long')
NO_MAP = ('below-cap', 'cap', 'cap+1', 'two', 'two-three', 'long')              # conv_b1_chain
STEM_CLASSES = tuple(STEM_NAMES)
C64_CLASSES = ('tpb1', 'tpb2-short', 'tpb3-short')
SUBOUT = tuple(f'two-three/w{w}-off{o}' for w in (16, 64) for o in (0, 1))      # in place of the plain `two-three`


def admitted_classes(inst):
    """The classes the instantiation's predicate admits (ADMITTED: the table the closure test of tests/test_kernel_coverage.py
    reads, which also asks the entry points by dry run whether `ragged` is true)."""
    if inst.family == 'c64':
        return C64_CLASSES
    if inst.family == 'stem':
        return STEM_CLASSES
    cls = STRIDED if inst.family in ('pw64', 'pws') else NO_MAP
    if 'subout' in inst.kid:
        cls = tuple(c for c in cls if c != 'two-three') + SUBOUT
    return cls + (('ragged-late',) if inst.ragged else ())


ADMITTED = {inst.kid: admitted_classes(inst) for inst in INSTANCES}
CASES = [(inst, cls) for inst in INSTANCES for cls in ADMITTED[inst.kid]]


def case_shape(inst, cls, cap):
    """(n, h, w, extra keywords of the builder, work items) of a class at grid cap `cap`."""
    g = (cap - cap % inst.halves) // inst.halves
    items = class_tiles(cls, g, cap)
    h, w = inst.tile_map
    extra = {}
    if '/' in cls:                      # two-three/w<width>-off<sub_off>
        width, off = cls.split('/')[1].split('-')
        extra['sub_off'] = int(off[3:])
        if width == 'w64':              # a tile is one map row of a W64_ROWS x 64 image
            assert items % W64_ROWS == 0, (cls, items)
            return items // W64_ROWS, W64_ROWS, 64, extra, items
    if cls == 'ragged-late':
        return 1, 1, (items - 1) * inst.tn + inst.tn - 5, extra, items
    return items, h, w, extra, items


# ---- one launch ------------------------------------------------------------------------------------------------------------------
_DRY = C.c_void_p(4096)


def _noted(lib):
    s = (C.c_int32 * 4)()
    check(lib.metro_last_launch_schedule(s), 'metro_last_launch_schedule')
    return lib.metro_last_kernel_id().decode().split(' & '), tuple(s)


def dry_run(lib, inst, cls, cap):
    """(ids, schedule record) of the case's launch at a grid cap of `cap`, without a device."""
    n, h, w, extra, items = case_shape(inst, cls, cap)
    pr = inst.build(n, min(n, BASE_IMAGES), h, w, **extra)
    check(lib.metro_kernel_notes(2), 'metro_kernel_notes')
    try:
        pr.launch(lib, {name: _DRY for name in list(pr.tensors) + list(pr.scratch)}, [_DRY] * len(pr.outs))
        return _noted(lib), items
    finally:
        lib.metro_kernel_notes(0)


def test_every_case_reaches_its_instantiation_without_a_gpu(lib):
    """Dry runs at a nominal cap of 256: the entry dispatches the instantiation the case names, with the work items of its class."""
    assert len(BY_ID) == len(INSTANCES)
    for inst, cls in CASES:
        (ids, sched), items = dry_run(lib, inst, cls, 256)
        assert tuple(ids) == inst.before + (inst.kid,), (inst.kid, cls, ids)
        assert sched == (items * inst.halves, items * inst.halves, 0, inst.halves), (inst.kid, cls, sched, items)


def _run(lib, cuda, inst, n, h, w, extra):
    px = n * h * w
    p = n if n <= BASE_IMAGES or (px * inst.macs <= REF_MACS and px * inst.elems <= REF_ELEMS) else BASE_IMAGES
    pr = inst.build(n, p, h, w, **extra)
    assign = H.crop_assignment(n, p, 11) if p < n else np.arange(n)
    dev = {}
    for name, a in pr.tensors.items():
        dev[name] = torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
        if name in pr.batched and p < n:
            dev[name] = H.lay_out_twins(dev[name], assign)
    for name, (shape, dt) in pr.scratch.items():
        dev[name] = torch.empty((n,) + shape, dtype=dt, device=cuda)
    guarded = [CC._guarded((n,) + shape, torch.float16, cuda) for shape in pr.outs]
    torch.cuda.synchronize()
    check(lib.metro_kernel_notes(1), 'metro_kernel_notes')
    try:
        pr.launch(lib, {k: H.ptr(v) for k, v in dev.items()}, [H.ptr(g[0]) for g in guarded])
        torch.cuda.synchronize()
        ids, sched = _noted(lib)
    finally:
        lib.metro_kernel_notes(0)
    return pr, p, assign, guarded, ids, sched


_CAPS = {}


def grid_cap(lib, cuda, inst):
    """The instantiation's grid cap on this device: what a first launch of the fewest work items records."""
    if inst.kid not in _CAPS:
        h, w = inst.tile_map
        _, _, _, _, ids, sched = _run(lib, cuda, inst, inst.min_items, h, w, {})
        assert tuple(ids) == inst.before + (inst.kid,), (inst.kid, ids)
        assert sched[2] > 0 and sched[3] == inst.halves and sched[1] == inst.min_items * inst.halves, (inst.kid, sched)
        _CAPS[inst.kid] = sched[2]
        print(f'\n[schedule] {inst.kid}: grid cap {sched[2]}, halves {inst.halves}, G {(sched[2] - sched[2] % inst.halves) // inst.halves}')
    return _CAPS[inst.kid]


@pytest.mark.gpu
@pytest.mark.parametrize('inst,cls', CASES, ids=[f'{i.kid}-{c}' for i, c in CASES])
def test_persistent_kernel_on_schedule(lib, cuda, inst, cls):
    cap = grid_cap(lib, cuda, inst)
    g = (cap - cap % inst.halves) // inst.halves
    assert g >= 16, f'{inst.kid}: a grid cap of {cap} leaves {g} tile streams: the classes below the cap need more than 8'
    n, h, w, extra, items = case_shape(inst, cls, cap)
    pr, p, assign, guarded, ids, sched = _run(lib, cuda, inst, n, h, w, extra)
    what = f'{inst.kid} {cls} ({n} x {h} x {w}, {items} work items, cap {cap}, G {g})'
    assert tuple(ids) == inst.before + (inst.kid,), f'{what}: launched {ids}'
    got, want = schedule_class(*sched, walk=inst.walk), expected_schedule(cls, g, cap)
    assert sched[1] == items * inst.halves and sched[2] == cap and sched[3] == inst.halves, f'{what}: recorded {sched}'
    assert matches(got, want), f'{what}: the launch {sched} is {got}, the class stands for {want}'
    if cls == 'ragged-late':
        assert (n * h * w) % inst.tn == inst.tn - 5 and items == -(-n * h * w // inst.tn)
    if '/' in cls:                      # what prev_sub -> now_sub does along the streams of THIS launch (recorded grid and work)
        moves = sub_store_transitions(sched[0], sched[1], h, w, extra['sub_off'])
        if w == 64:
            assert {(4, 0), (0, 4)} <= moves, (f'{what}: no stream runs a tile without sub-sampled stores behind one with all of them '
                                               f'and the reverse (prev_sub -> now_sub takes {sorted(moves)})')
        else:
            assert moves == {(2, 2)}, f'{what}: prev_sub -> now_sub takes {sorted(moves)}'
        what += f', prev_sub -> now_sub in {sorted(moves)}'
    ts = pr.tensors
    with np.errstate(all='ignore'):
        ref = pr.ref(ts)
    worst = 0.0
    for k, ((out, buf), r) in enumerate(zip(guarded, ref)):
        assert CC._guards_intact(buf), f'{what}, output {k}: a store landed outside the tensor'
        assert bool(torch.isfinite(out).all()), f'{what}, output {k}: {int((~torch.isfinite(out)).sum())} elements not written (or not finite)'
        if p < n:
            H.assert_twins(out, assign, p, f'{what}, output {k}')
        err = np.abs(out[:p].cpu().numpy().astype(f64) - r.exact)
        bad = ~(err <= r.bound)
        ratio = float((err / np.maximum(r.bound, 1e-300)).max())
        worst = max(worst, ratio)
        assert not bad.any(), (f'{what}, output {k}: {int(bad.sum())} of {bad.size} elements out of bound; worst {ratio:.3g} x the bound, '
                               f'first at {tuple(int(v) for v in np.argwhere(bad)[0])}')
    print(f'\n[schedule] {what}: grid {sched[0]}, streams {got.streams}, tiles per stream {got.t_min}..{got.t_max} ({got.n_max} run the most), '
          f'{got.branch} map, {"every pixel" if p == n else f"{p} base images + twins"} held to fp64, worst error {worst:.3f} x the bound')
