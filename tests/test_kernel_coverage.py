"""Every kernel INSTANTIATION a BASELINE configuration dispatches at its per-GPU batch, against the fp64 reference.

Which kernel a layer runs on depends on its shape and on the batch (tile counts against the 256 CUs): parity shown for a
layer at n = 1 says nothing about the instantiation the same layer gets at n = 32.  `metro_plan_layer_kernel` names the
instantiation (a dry run of the dispatch, no device needed), so this file can

  * (CPU) enumerate the ids of C1..C5 (+ the north star's batch 256) without a GPU, and
  * (`-m gpu`) for EVERY distinct id of every configuration take the first layer that dispatches it and run that layer's
    real shape at the configuration's real batch through the single-kernel C-ABI entry point, check that the entry
    point launched exactly the instantiation the plan names (`metro_last_kernel_id`), and compare with the fp64 reference
    on the same fp16 operands (2e-3 of the layer maximum = fp16 output rounding; reference resnet_v2.py:119-138,219-236,
    resnet_utils.py:82-135, volumetric.py:227-235).  The batch is built from FOUR images: the reference is computed for
    them, at positions 0..3, and every other position must carry the same bits as its twin.  Which image a position holds
    is drawn so that no shift of the sequence, no rotation of the batch and no swap of two adjacent aligned groups of 2, 4,
    8 or 16 images maps the layout onto itself (tests/helpers.py: crop_assignment; tests/test_crop_assignment.py plants such
    faults): a launch that stores whole tiles into other tiles' slots -- with image i = image i mod 4 it would give every
    position "its twin's bits" whenever it moves results by a multiple of four images -- fails the twin check, so each tile
    position of the launch is held to the oracle at the cost of four images.
  * (`-m gpu`) the same for single launches (spec, batch, layer): the instantiations that only call sizes off the powers of two
    reach (SINGLE_LAUNCHES), and every (kernel id, layer shape) pair of the released models' crop side that the cases above do
    not launch -- the list comes from the dry run over every call size 1 .. 256 that the two CPU closure tests make.
"""
import ctypes as C
import hashlib
import json
import os
import zlib

import numpy as np
import pytest
import torch

from metro_pose3d_amd import ModelSpec, _lib
from metro_pose3d_amd._lib import check
from metro_pose3d_amd.engine import Engine
from tests import helpers as H

# BASELINE.json configs at their per-GPU batch (configs[2..4] are sharded 8 ways: 512/8, 256/8, 128/8) + the north star's batch
CONFIGS = {
    'C1-rn50-s32-J17-b1': (ModelSpec(50, 32, 'h36m'), 1),
    'C2-rn50-s16-J17-b64': (ModelSpec(50, 16, 'h36m'), 64),
    'C2-rn50-s16-J17-b256': (ModelSpec(50, 16, 'h36m'), 256),
    'C3-rn50-s16-J19-b64': (ModelSpec(50, 16, 'many19'), 64),
    'C3-rn50-s16-J19-b256': (ModelSpec(50, 16, 'many19'), 256),       # 152 head channels: the 160 x 256 head (whole K per wave)
    'C4-rn101-s8-J19-b32': (ModelSpec(101, 8, 'many19'), 32),
    'C5-rn50-s4-J17-b16': (ModelSpec(50, 4, 'h36m'), 16),
    # not BASELINE configurations: head shapes the ring head kernel would otherwise never see in a test -- depth 4 (the generic
    # statistics path: five-joint batches are for depth 8) and 128-pixel tiles with 144 weight rows (17 joints at stride 8)
    'X-rn50-s16-J17-D4-b64': (ModelSpec(50, 16, 'h36m', depth=4), 64),
    'X-rn50-s8-J17-b32': (ModelSpec(50, 8, 'h36m'), 32),
    # estimate_pose's middle bucket: block4's conv1 on conv_gemm4w QUARTER tiles (256 cout x 64 px, round 6), block4's pair at 1.25 rounds
    'X-rn50-s16-J17-b32': (ModelSpec(50, 16, 'h36m'), 32),
    # the released `many_*` exports: the 53-joint `merged` head = 424 channels (reference data/datasets.py:142-154, main.py:119-127)
    # in three joint groups on the ring head (round 5), 64- and 128-pixel tiles
    'X-rn50-s16-merged53-b64': (ModelSpec(50, 16, 'merged'), 64),
    'X-rn101-s8-merged53-b32': (ModelSpec(101, 8, 'merged'), 32),
    # estimate_pose's batch-256 bucket at stride 32: block3/unit_6/conv3 on the 128 x 256 ring tiles with a residual
    'X-rn50-s32-J17-b256': (ModelSpec(50, 32, 'h36m'), 256),
    # ---- crop sides other than 256 (the model file's proc_side): maps that are not powers of two, heads that are not whole tiles
    # 224: 56/28/14/7-wide maps; the 7 x 7 head is not whole 64-pixel tiles -> the f32out GEMM and the two-launch soft-argmax
    'X-rn50-s32-J17-side224-b64': (ModelSpec(50, 32, 'h36m', proc_side=224), 64),
    # 288: an 18 x 18 heat map of the 424-channel head (2 pixel lanes per soft-argmax block)
    'X-rn50-s16-merged53-side288-b64': (ModelSpec(50, 16, 'merged', proc_side=288), 64),
    # 384: 96/48/24-wide maps, the one-launch head on a 24 x 24 heat map (32-pixel slabs cross image rows)
    'X-rn50-s16-J17-side384-b64': (ModelSpec(50, 16, 'h36m', proc_side=384), 64),
    # 320: 80/40-wide maps; the 256-pixel head on an 80 x 80 heat map, and RN101-s8's 40 x 40 head
    'X-rn101-s8-J19-side320-b32': (ModelSpec(101, 8, 'many19', proc_side=320), 32),
    'X-rn50-s4-J17-side320-b16': (ModelSpec(50, 4, 'h36m', proc_side=320), 16),
    # 512: block1 on 128-wide maps (the 512-row slab of the tap-reuse 3x3), and at stride 4 its sub-grid form on a 128 x 128 head
    'X-rn50-s32-J17-side512-b1': (ModelSpec(50, 32, 'h36m', proc_side=512), 1),
    'X-rn50-s4-J17-side512-b1': (ModelSpec(50, 4, 'h36m', proc_side=512), 1),
    # the cheapest shapes of the remaining instantiations: 64 px (16-wide block1, a 4 x 4 head of 424 channels: 128 x 128 f32out
    # GEMM, block4's conv3 on the weight-resident 1x1), 416 px at stride 8 (block4 on 52-wide maps: the 256 x 256 ring pair, the
    # 128 x 256 deep-K conv1)
    'X-rn50-s16-merged53-side64-b1': (ModelSpec(50, 16, 'merged', proc_side=64), 1),
    'X-rn50-s8-J17-side416-b8': (ModelSpec(50, 8, 'h36m', proc_side=416), 8),
}
BASE_IMAGES = 4                 # distinct images of a batch: the oracle's cost per case

# The supported range of the f16 path (test_dispatch_closure): every plan of this grid dispatches only instantiations that a GPU
# test launches at some shape
GRID_SIDES = range(64, 513, 32)
GRID_ARCHS = (50, 101)
GRID_STRIDES = (4, 8, 16, 32)
GRID_DATASETS = ('h36m', 'many19', 'merged')
GRID_BATCHES = range(1, 257)    # every call size: estimate_pose forwards what it is given, the frames chain calls with boxes x views crops

# Single launches away from proc_side 256: (spec, batch, layer) at the cheapest shape of the grid that reaches an instantiation
# no configuration above and no test_f16_layerwise case dispatches -- both are reached at call sizes off the powers of two only.
# (Not CONFIGS entries: a configuration adds a case per id it dispatches, and at 4 crops of side 512 those are fifteen more
# launches on 128 x 128 maps, ~490 GFLOP of fp64 reference for ids that are held elsewhere.)
SINGLE_LAUNCHES = [
    # conv_igemm_f16_dma<256x256,bk32,s4,pro>: the conv1 layers of block3 / block4 (1024 -> 256, 2048 -> 512) once the call has
    # ~250 tiles of 256 pixels, e.g. RN50-s4 at side 224 from 11 crops on.  Here 135 crops of 22 x 22 maps: 65 340 pixels, the last
    # of 256 tiles holds 60 of them
    (ModelSpec(50, 16, 'h36m', proc_side=352), 135, 'block3/unit_2/conv1'),
    # conv3x3_f16_slab<128x256,rows384,...>+subgrid: block2's rate-2 3x3 at stride 4 on 128 x 128 maps, at 4..7 crops only
    # (fewer: 64-cout tiles; more: 512-pixel tiles).  4 crops: all four positions held to fp64 themselves
    (ModelSpec(50, 4, 'h36m', proc_side=512), 4, 'block2/unit_1/conv2'),
]

# The (kernel id, layer shape) closure (test_pair_closure): the released models' crop side, every arch / stride / head, every call size
PAIR_SPECS = [ModelSpec(a, s, d) for a in GRID_ARCHS for s in GRID_STRIDES for d in GRID_DATASETS]
# what a launch's runtime arguments (K-loop length, halo, dilation, map side, residual form, fused outputs) are made of
SHAPE_KEY = ('kind', 'c_in', 'c_out', 'h_in', 'h_out', 'kh', 'stride', 'dilation', 'relu', 'has_residual', 'res_stride', 'res_offset',
             'has_prologue', 'out_dtype', 'fused_flags', 'out2_channels')


def shape_key(li):
    return tuple(getattr(li, f) for f in SHAPE_KEY)


def spec_name(spec):
    return f'rn{spec.arch}-s{spec.stride}-{spec.dataset}' + ('' if spec.proc_side == 256 else f'-side{spec.proc_side}')


def dispatch_table(spec, n):
    """[(layer index, MetroLayerInfo, kernel id)] of an f16 plan at batch n -- no GPU needed."""
    eng = Engine(spec, None, 'f16', max_batch=n)
    return list(zip(range(10 ** 6), eng.layer_infos(), eng.layer_kernels(n)))


class DryRun:
    """The dispatch of one spec at every batch up to max_batch from ONE plan (max_batch sizes the workspace slots and nothing else
    of a plan; test_dispatch_closure holds that against dispatch_table for every configuration).  kernels(n, layers): the ids of
    the given layer indices (all by default).  `precision`: the plan's mode (tests/test_parity_coverage.py walks the parity modes)."""

    def __init__(self, spec, max_batch=256, precision='f16'):
        self.spec = spec
        self.eng = Engine(spec, None, precision, max_batch=max_batch)
        self.infos = self.eng.layer_infos()
        self.names = [li.name.decode() for li in self.infos]
        self.keys = [shape_key(li) for li in self.infos]
        self._buf = C.create_string_buffer(1024)

    def kernels(self, n, layers=None):
        out = []
        for i in range(len(self.infos)) if layers is None else layers:
            check(self.eng.lib.metro_plan_layer_kernel(self.eng._plan, i, int(n), self._buf, len(self._buf)), 'metro_plan_layer_kernel')
            out.append(self._buf.value.decode())
        return out


def _first_layers_by_id():
    out = []
    for cname, (spec, n) in CONFIGS.items():
        seen = set()
        for i, li, kid in dispatch_table(spec, n):
            if kid not in seen:
                seen.add(kid)
                out.append(pytest.param(cname, i, kid, id=f'{cname}:{li.name.decode()}:{kid}'))
    return out


def _layerwise_runs():
    """(who, spec, batch) of every test_f16_layerwise case: each launches every layer of its plan at its real batch."""
    from tests.test_f16_layerwise import CASES
    return [(f'test_f16_layerwise[{i}]', c[0], c[2].get('batch', c[1]) if len(c) > 2 else c[1]) for i, c in enumerate(CASES)]


def _launched_by(table, layer):
    """The layers of a dispatch table that a case on `layer` launches: the one-launch head takes its finalize with it (_head)."""
    _, li, kid = table[layer]
    both = li.name == b'logits' and kid.startswith('head_f16')
    return [layer, layer + 1] if both else [layer]


def launched_pairs(config_cases, single_cases):
    """{(kernel id, shape key): who} of what the GPU cases launch: of every configuration the layers its cases name (the first per
    id, not the whole plan), every layer of the test_f16_layerwise cases, and the single launches (spec, batch, layer index)."""
    out = {}
    tables = {}
    for p in config_cases:
        cname, layer, _ = p.values
        if cname not in tables:
            tables[cname] = dispatch_table(*CONFIGS[cname])
        for i in _launched_by(tables[cname], layer):
            out.setdefault((tables[cname][i][2], shape_key(tables[cname][i][1])), cname)
    for who, spec, n in _layerwise_runs():
        for _, li, kid in dispatch_table(spec, n):
            out.setdefault((kid, shape_key(li)), who)
    for p in single_cases:
        spec, n, layer, _ = p.values
        table = dispatch_table(spec, n)
        for i in _launched_by(table, layer):
            out.setdefault((table[i][2], shape_key(table[i][1])), p.id)
    return out


_UNIVERSE = {}


def pair_universe():
    """{(kernel id, shape key): (spec, n, layer index)} over PAIR_SPECS x GRID_BATCHES: the point with the smallest n (then the
    first spec) that reaches each pair.  One dry run per process, shared by the case list below and test_pair_closure."""
    if not _UNIVERSE:
        for spec in PAIR_SPECS:
            run = DryRun(spec)
            for n in GRID_BATCHES:
                for i, kid in enumerate(run.kernels(n)):
                    at = _UNIVERSE.get((kid, run.keys[i]))
                    if at is None or n < at[1]:
                        _UNIVERSE[(kid, run.keys[i])] = (spec, n, i)
    return _UNIVERSE


def _single_param(spec, n, layer, kid, name):
    return pytest.param(spec, n, layer, kid, id=f'{spec_name(spec)}-b{n}:{name}:{kid}')


def _single_launches():
    """SINGLE_LAUNCHES, then for every pair of the universe that no configuration case and no test_f16_layerwise case launches the
    (spec, smallest n, layer) that reaches it.  A head's finalize launch comes with the head case of the same (spec, n)."""
    out = []
    for spec, n, name in SINGLE_LAUNCHES:
        table = dispatch_table(spec, n)
        i = [li.name.decode() for _, li, _ in table].index(name)
        out.append(_single_param(spec, n, i, table[i][2], name))
    have = launched_pairs(_CASES, out)
    todo = sorted(((spec_name(spec), n, i), pair) for pair, (spec, n, i) in pair_universe().items() if pair not in have)
    specs = {spec_name(s): s for s in PAIR_SPECS}
    for (sname, n, i), pair in todo:        # in (spec, n, layer) order: a head in front of its finalize
        if pair in have:
            continue
        spec = specs[sname]
        table = dispatch_table(spec, n)
        if table[i][1].name == b'softargmax' and pair[0] == 'softargmax_finalize<acc32>':
            i -= 1                          # launched by the head in front of it
        out.append(_single_param(spec, n, i, table[i][2], table[i][1].name.decode()))
        for k in _launched_by(table, i):
            have.setdefault((table[k][2], shape_key(table[k][1])), out[-1].id)
    return out


try:
    _CASES = _first_layers_by_id()
    _SINGLE_CASES = _single_launches()
except Exception as e:  # noqa: BLE001  (library not built: the CPU test below reports it)
    _CASES = [pytest.param(None, -1, str(e), id='library-missing')]
    _SINGLE_CASES = [pytest.param(None, 0, -1, str(e), id='library-missing')]


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_every_layer_names_its_kernel_without_a_gpu():
    ids = {}
    for cname, (spec, n) in CONFIGS.items():
        table = dispatch_table(spec, n)
        assert all(kid and '<' in kid or kid in ('conv3x3_c64', 'prep_input_f16') for _, _, kid in table), [k for _, _, k in table]
        ids[cname] = {li.name.decode(): kid for _, li, kid in table}
    # the choice depends on the batch: RN101-s8 block3 conv2 (256 ch, rate 2, 32x32) takes 128-cout x 256-px tiles with a
    # 64-row halo at batch 32 and 64-cout tiles at batch 1
    assert ids['C4-rn101-s8-J19-b32']['block3/unit_2/conv2'] == 'conv3x3_f16_slab<128x256,rows384,bufs2,tps1,kc64,ws3>'
    small = {li.name.decode(): kid for _, li, kid in dispatch_table(ModelSpec(101, 8, 'many19'), 1)}
    assert small['block3/unit_2/conv2'] != ids['C4-rn101-s8-J19-b32']['block3/unit_2/conv2']
    # round 6: the rate-4 / rate-8 3x3 layers of strides 4 and 8 run on the tap-reuse kernel in sub-grid pixel order (they fell to the ring kernel
    # before); block4's conv1 at 64 crops on conv_gemm4w HALF tiles, its shortcut + conv1 pair as whole + half tiles in one grid; at 32 crops
    # QUARTER tiles; RN101-s8's block3 conv1 at 32 crops on half tiles
    assert ids['C5-rn50-s4-J17-b16']['block4/unit_2/conv2'] == 'conv3x3_f16_slab<128x512,rows640,bufs2,tps1,kc32,ws4>+subgrid'
    assert ids['C5-rn50-s4-J17-b16']['block3/unit_2/conv2'].endswith('+subgrid') and ids['C4-rn101-s8-J19-b32']['block4/unit_2/conv2'].endswith('+subgrid')
    assert not any(k.startswith('conv_igemm_f16_dma') for n_, k in ids['C5-rn50-s4-J17-b16'].items() if n_.endswith('/conv2') and ('block3' in n_ or 'block4' in n_))
    assert '+subgrid' not in ids['C2-rn50-s16-J17-b64']['block4/unit_2/conv2']        # rate 2 on 16 x 16: the plain order (measured faster)
    assert ids['C2-rn50-s16-J17-b64']['block4/unit_2/conv1'] == 'conv_gemm4w<256x128,pro>'
    assert ids['C2-rn50-s16-J17-b64']['block4/unit_1/shortcut+conv1'] == 'conv_gemm4w<256x256,pro>+pair & conv_gemm4w<256x128,pro>+pair'
    assert ids['C2-rn50-s16-J17-b256']['block4/unit_2/conv1'] == 'conv_gemm4w<256x256,pro>'
    assert ids['C2-rn50-s16-J17-b256']['block4/unit_1/shortcut+conv1'] == 'conv_gemm4w<256x256,pro>+pair'
    assert ids['X-rn50-s16-J17-b32']['block4/unit_2/conv1'] == 'conv_gemm4w<256x64,pro>'
    assert ids['C4-rn101-s8-J19-b32']['block3/unit_2/conv1'] == 'conv_gemm4w<256x128,pro>'
    # the one-launch head and its finalize
    # (head_f16.hip: tile width by the number of tiles, weight rows by the head's channels, K-parts per wave group)
    assert ids['C1-rn50-s32-J17-b1']['logits'] == ids['C2-rn50-s16-J17-b64']['logits'] == 'head_f16<144x64,k4>'
    assert ids['C3-rn50-s16-J19-b64']['logits'] == 'head_f16<160x64,k4>'
    assert ids['C4-rn101-s8-J19-b32']['logits'] == 'head_f16<160x128,k4>'
    assert ids['C2-rn50-s16-J17-b256']['logits'] == ids['C5-rn50-s4-J17-b16']['logits'] == 'head_f16<144x256,k2>'
    assert ids['C3-rn50-s16-J19-b256']['logits'] == 'head_f16<160x256>'
    assert ids['X-rn50-s16-J17-D4-b64']['logits'] == 'head_f16<144x64,k4>' and ids['X-rn50-s8-J17-b32']['logits'] == 'head_f16<144x128,k4>'
    assert ids['X-rn50-s16-merged53-b64']['logits'] == 'head_f16<160x64,k4,g3>' and ids['X-rn101-s8-merged53-b32']['logits'] == 'head_f16<160x128,k4,g3>'
    assert ids['X-rn50-s16-merged53-b64']['softargmax'] == 'softargmax_finalize<acc32>'
    assert ids['C2-rn50-s16-J17-b64']['softargmax'] == 'softargmax_finalize<acc32>'
    # parity modes name their kernels too
    e64 = Engine(ModelSpec(50, 16, 'h36m'), None, 'f64', max_batch=2)
    k64 = e64.layer_kernels(2)
    assert k64[0].startswith('conv_igemm_f64acc<') and k64[-1] == 'softargmax_partial<acc64,logits64> & softargmax_finalize<acc64>'
    k32 = Engine(ModelSpec(50, 16, 'h36m'), None, 'f32m', max_batch=2).layer_kernels(2)
    assert k32[0] == 'conv_igemm_f32<64x128,bk32>' and k32[3].startswith('conv_igemm_f32<') and ',v4' in k32[3]
    assert k32[-1] == 'softargmax_partial<acc64,logits32> & softargmax_finalize<acc64>'
    # crop sides other than 256: a 56-wide 3x3 takes neither the tap-reuse slab kernel (256 % W) nor conv3x3_c64 (128 % W)
    s224 = ids['X-rn50-s32-J17-side224-b64']
    for name in ('block1/unit_1/conv2', 'block1/unit_2/conv2', 'block1/unit_3/conv2'):
        assert s224[name].startswith('conv_igemm_f16_dma<'), (name, s224[name])
    # a 7 x 7 head is not whole 64-pixel tiles: the fp32-output GEMM, then the two-launch soft-argmax
    assert s224['logits'] == 'conv_igemm_f16_dma<64x128,bk64,s3,pro>+f32out'
    assert s224['softargmax'] == 'softargmax_partial<acc32,logits32> & softargmax_finalize<acc32>'
    assert ids['X-rn50-s16-merged53-side288-b64']['logits'] == 'conv_igemm_f16_dma<128x256,bk64,s3,pro>+f32out'
    assert ids['X-rn50-s16-merged53-side64-b1']['logits'] == 'conv_igemm_f16_dma<128x128,bk64,s4,pro>+f32out'
    # ... a 24 x 24 one is 9 tiles: the one-launch head, as is 80 x 80 on 256-pixel tiles and 40 x 40 on 128-pixel ones
    assert ids['X-rn50-s16-J17-side384-b64']['logits'] == 'head_f16<144x64,k4>'
    assert ids['X-rn50-s16-J17-side384-b64']['softargmax'] == 'softargmax_finalize<acc32>'
    assert ids['X-rn50-s4-J17-side320-b16']['logits'] == 'head_f16<144x256,k2>'
    assert ids['X-rn101-s8-J19-side320-b32']['logits'].startswith('head_f16<160x')
    # 128-wide block1 maps: the 512-row slab of the tap-reuse 3x3; at stride 4 the rate-2 block3 on its sub-grid form
    assert ids['X-rn50-s32-J17-side512-b1']['block1/unit_1/conv2'] == 'conv3x3_f16_slab<64x256,rows512,bufs2,tps1,kc64,ws3>'
    assert ids['X-rn50-s4-J17-side512-b1']['block1/unit_1/conv2'] == 'conv3x3_f16_slab<64x256,rows512,bufs2,tps1,kc64,ws3>'
    # the stem of any side but 256 reads its fp32 image without the side-256 specialisation
    assert all(ids[c]['conv1+pool1'] == 'stem_pool_f16<split2,f32in>' for c in ids if '-side' in c)


def _gpu_tested_ids(single_cases=None):
    """Every kernel id a GPU test launches: the CONFIGS above (this file), the layer-by-layer cases of test_f16_layerwise.py, each
    at its real batch, and the single launches."""
    out = {}
    for who, spec, n in [(c, s, n) for c, (s, n) in CONFIGS.items()] + _layerwise_runs():
        for k in Engine(spec, None, 'f16', max_batch=n).layer_kernels(n):
            out.setdefault(k, who)
    for p in _SINGLE_CASES if single_cases is None else single_cases:
        out.setdefault(p.values[3], p.id)
    return out


def _same_backbone(a, b):
    """The layers in front of the head of two plans that differ in the head only: same names, same shapes, same fused forms."""
    skip = ('name', 'out_offset', 'out2_offset', 'out_sub_offset')        # (slot offsets follow the head's size)
    fields = [f for f, _ in _lib.MetroLayerInfo._fields_ if f not in skip]
    la, lb = a.names.index('logits'), b.names.index('logits')
    return la == lb and a.names == b.names and \
        all(getattr(x, f) == getattr(y, f) for x, y in zip(a.infos[:la], b.infos[:lb]) for f in fields)


def test_dispatch_closure():
    """The supported range of the f16 path is the grid

        proc_side 64, 96, ..., 512  x  ResNet-v2 50 / 101  x  stride 4 / 8 / 16 / 32  x  h36m / many19 / merged heads
        x  EVERY batch 1 .. 256

    (a dry run of the dispatch: no device).  Every kernel instantiation a plan of this grid dispatches must be launched by a
    GPU test -- a configuration of CONFIGS, a test_f16_layerwise case at its real batch, or a single launch -- so no shape of
    the range reaches a kernel no test has held to the fp64 reference.  The batches are not sampled: which kernel a layer runs
    on turns on tile counts against the 256 CUs, and two instantiations of this grid are reached at no power of two.

    The scan is whole: 408 specs x 256 batches, one plan per spec.  The many19 and merged specs are asked for their head
    layers only, after the assertion that every layer in front of their head equals h36m's (metro_plan_layer_kernel is per
    layer).  Measured: 8 s on the build machine (24 s with every layer of every spec)."""
    tested = _gpu_tested_ids()
    # one plan serves every batch: the ids it names are those of a plan made for exactly that batch
    for cname, (spec, n) in CONFIGS.items():
        assert DryRun(spec).kernels(n) == [k for _, _, k in dispatch_table(spec, n)], cname
    untested = {}
    for side in GRID_SIDES:
        for arch in GRID_ARCHS:
            for stride in GRID_STRIDES:
                base = None
                for ds in GRID_DATASETS:
                    run = DryRun(ModelSpec(arch, stride, ds, proc_side=side))
                    layers = None
                    if base is None:
                        base = run
                    else:
                        assert _same_backbone(base, run), f'rn{arch}-s{stride}-{ds} at proc_side {side}: backbone differs from {base.spec.dataset}\'s'
                        layers = range(run.names.index('logits'), len(run.names))
                    for n in GRID_BATCHES:
                        for k in run.kernels(n, layers):
                            if k not in tested:
                                untested.setdefault(k, f'rn{arch}-s{stride}-{ds} at proc_side {side}, batch {n}')
    assert not untested, 'dispatched by the supported grid but launched by no GPU test (first plan that reaches it):\n' + \
        '\n'.join(f'  {k}: {w}' for k, w in sorted(untested.items()))


def test_pair_closure():
    """One level below test_dispatch_closure: an instantiation's runtime arguments (K-loop length, halo, dilation, map side,
    residual form, fused outputs) come from the layer, so an id that is right on one layer shape can be wrong on another
    (the sub-grid 3x3 on a layer beyond its slab was).  Every (kernel id, layer shape) pair -- the shape is SHAPE_KEY of
    MetroLayerInfo -- that the released models' crop side dispatches,

        proc_side 256  x  ResNet-v2 50 / 101  x  stride 4 / 8 / 16 / 32  x  h36m / many19 / merged heads  x  every batch 1 .. 256,

    must be LAUNCHED by a GPU case: the layer a configuration's case names (the first per id, not its whole plan), any layer of
    a test_f16_layerwise case at its real batch, or a single launch.  The stated limit: other crop sides stay at the level of
    ids (test_dispatch_closure) -- the whole grid has some 1 700 pairs, most of which differ in the map side only."""
    universe = pair_universe()
    tested = launched_pairs(_CASES, _SINGLE_CASES)
    print(f'\n{len(universe)} (kernel id, layer shape) pairs at proc_side 256; {len(tested)} pairs launched by the GPU cases '
          f'({len(_CASES)} configuration cases, {len(_layerwise_runs())} layer-by-layer cases, {len(_SINGLE_CASES)} single launches)')
    missing = {pair: at for pair, at in universe.items() if pair not in tested}
    assert not missing, 'dispatched at proc_side 256 but launched by no GPU case (kernel id: the smallest call that reaches the shape):\n' + \
        '\n'.join(f'  {kid}: {spec_name(spec)}, batch {n}, {DryRun(spec, n).names[i]} {dict(zip(SHAPE_KEY, key))}'
                  for (kid, key), (spec, n, i) in sorted(missing.items(), key=lambda kv: (kv[0][0], kv[1][1])))


# ---- operands beyond 2^31 / 2^32 bytes and beyond 2^31 elements ------------------------------------------------------------------
# class -> (unit, boundary): an operand is in the class when its size in that unit is BEYOND the boundary (strictly: a tensor of
# exactly 2^32 bytes has no byte whose offset needs bit 32)
LARGE_CLASSES = {'A': ('bytes', 2 ** 31), 'B': ('bytes', 2 ** 32), 'E': ('elements', 2 ** 31)}
LARGE_ROLES = ('input', 'output', 'second output', 'residual', 'sub-sampled output', 'fp32 logits')
LARGE_IMAGES_BEYOND = 4         # whole images a case puts beyond the boundary of every triple it is there for (fewer only at n = 256)
DTYPE_BYTES = {_lib.METRO_F16: 2, _lib.METRO_F32: 4, _lib.METRO_F64: 8}


def large_kernel_names(kid):
    """The kernels of an id for the large-operand closure: kernel_of (tests/test_gpu_nonfinite_kernels.py) of every part of an
    `a & b` id, with the form suffix behind the template arguments (+pair, +subgrid, +f32out, +res) kept."""
    from tests.test_gpu_nonfinite_kernels import kernel_of
    return sorted({kernel_of(part) + (part[part.rindex('>') + 1:] if '>' in part else '') for part in kid.split(' & ')})


def operand_roles(infos, i, kid):
    """{role: (elements per image, bytes per element)} of the tensors the launch of layer i touches that grow with the call size
    (the roles of LARGE_ROLES; weights, the 64-channel side inputs of block1's rebuilt shortcuts, soft-argmax records and poses do
    not reach 2^31 bytes at 256 crops).  The element size comes from the layer's dtypes: the stem reads the fp32 image, every other
    layer what the layer in front stores (the plan's activation type; the two-launch soft-argmax the logits' type)."""
    li = infos[i]
    name = li.name.decode()
    act = DTYPE_BYTES[infos[0].out_dtype]
    out_b = DTYPE_BYTES[li.out_dtype]
    px = li.h_out * li.w_out
    if li.kind == _lib.LAYER_SOFTARGMAX:       # the finalize launch behind the one-launch head reads records, not logits
        return {'input': (li.h_in * li.w_in * li.c_in, DTYPE_BYTES[infos[i - 1].out_dtype])} if 'softargmax_partial' in kid else {}
    if name == 'conv1+pool1':                   # (h_in, c_in of this layer describe the padded slab; the image is 4 h_out wide, 3 channels)
        return {'input': (16 * px * 3, 4), 'output': (px * li.c_out, out_b)}
    roles = {'input': (li.h_in * li.w_in * li.c_in, 4 if name == 'conv1' else act)}
    if name == 'logits' and kid.startswith('head_f16'):
        roles['fp32 logits'] = (px * li.c_out, 4)          # what the single launch stores next to the poses (metro_forward keeps them on chip)
        return roles
    if li.kind != _lib.LAYER_CONV:
        roles['output'] = (px * li.c_in if li.kind == _lib.LAYER_POOL else px * li.c_out, out_b)
        return roles
    if not li.fused_flags & _lib.FUSED_OUT_ON_CHIP:
        roles['output'] = (px * li.c_out, out_b)
    if li.out2_channels > 0 and not li.fused_flags & _lib.FUSED_CONV1_IN_FRONT:
        roles['second output'] = (px * li.out2_channels, act)
    if li.has_residual and not li.fused_flags & _lib.FUSED_REBUILT_SHORTCUT:
        whole = li.res_stride == 1 or li.fused_flags & _lib.FUSED_COMPACT_SHORTCUT
        roles['residual'] = ((px if whole else 4 * px) * li.c_out, out_b)
    if li.out_sub_offset >= 0:
        roles['sub-sampled output'] = (li.out_sub_side ** 2 * li.c_out, out_b)
    return roles


def images_beyond(n, per_image, bound):
    """Whole images of a tensor of n images, per_image units each, that lie beyond `bound` units: image i does when i * per_image >= bound."""
    return max(0, n - -(-bound // per_image))


def large_triples(infos, i, kid, n):
    """{(kernel, role, class): whole images beyond the class's boundary} of layer i at call size n; only operands IN the class."""
    out = {}
    for role, (elems, width) in operand_roles(infos, i, kid).items():
        for cls, (unit, bound) in LARGE_CLASSES.items():
            per = elems * width if unit == 'bytes' else elems
            if n * per > bound:
                for k in large_kernel_names(kid):
                    out[(k, role, cls)] = images_beyond(n, per, bound)
    return out


_LARGE = {}


def large_operand_scan(precision='f16'):
    """[(multiply-accumulates, precision, spec, n, layer index, kernel id, {triple: images beyond})]: every (spec, n, layer) of the
    supported grid (GRID_SIDES x GRID_ARCHS x GRID_STRIDES x GRID_DATASETS x GRID_BATCHES) with an operand beyond 2^31 bytes.
    Operands grow with n: per spec the walk goes down from 256, asks only for the layers whose largest operand is beyond 2^31
    bytes at that n, and stops at the first n with none (a spec whose plan has none at 256 costs one plan); the many19 and merged
    specs are asked for their head layers only (test_dispatch_closure asserts that their backbones are h36m's)."""
    if precision in _LARGE:
        return _LARGE[precision]
    found = []
    for side in GRID_SIDES:
        for arch in GRID_ARCHS:
            for stride in GRID_STRIDES:
                for ds in GRID_DATASETS:
                    spec = ModelSpec(arch, stride, ds, proc_side=side)
                    run = DryRun(spec, precision=precision)
                    layers = range(0 if ds == GRID_DATASETS[0] else run.names.index('logits'), len(run.names))
                    # the largest operand of a layer whatever kernel it gets (the head's fp32 logits, the two-launch soft-argmax's input)
                    largest = {i: max(e * w for kid in ('', 'head_f16<', 'softargmax_partial<')
                                      for e, w in operand_roles(run.infos, i, kid).values()) for i in layers}
                    for n in reversed(GRID_BATCHES):
                        ask = [i for i in layers if n * largest[i] > 2 ** 31]
                        if not ask:
                            break
                        for i, kid in zip(ask, run.kernels(n, ask)):
                            t = large_triples(run.infos, i, kid, n)
                            if t:
                                found.append((run.infos[i].flops_per_image / 2 * n, precision, spec, n, i, kid, t))
    _LARGE[precision] = found
    return found


def large_universe(scan):
    """Every triple the scan reaches."""
    return {t for c in scan for t in c[6]}


def _holds(n, images):
    """Whether a launch at call size n holds a triple: LARGE_IMAGES_BEYOND whole images beyond the boundary, or the grid's largest call."""
    return images >= LARGE_IMAGES_BEYOND or n == GRID_BATCHES[-1]


def held_triples(n, triples):
    return {t for t, images in triples.items() if _holds(n, images)}


def large_address_cases(scan):
    """The case list: [(precision, spec, n, layer index, kernel id, {triple: images beyond} the case is there for)].  For every
    triple not yet held -- classes E, B, A in that order, one launch usually holds several roles and classes -- the (spec, n,
    layer) with the fewest multiply-accumulates that holds it (fewest for a layer = its smallest n with LARGE_IMAGES_BEYOND images
    beyond; ties: ResNet-50, the smaller stride and side); everything else that launch holds is then held.  A triple that no
    point of the grid holds (its kernel leaves the layer before four images lie beyond) goes to the point with the most images
    beyond."""
    order = sorted(large_universe(scan), key=lambda t: ('EBA'.index(t[2]), t[0], t[1]))
    cost = lambda c: (c[0], c[2].arch, c[2].stride, c[2].proc_side, c[2].dataset, c[1], c[3], c[4])
    held, cases = set(), []
    for t in order:
        if t in held:
            continue
        at = [c for c in scan if t in c[6]]
        good = [c for c in at if _holds(c[3], c[6][t])]
        _, prec, spec, n, i, kid, triples = min(good, key=cost) if good else max(at, key=lambda c: (c[6][t], -c[0]))
        mine = {u: k for u, k in triples.items() if (_holds(n, k) or u == t) and u not in held}
        held.update(mine)
        cases.append((prec, spec, n, i, kid, mine))
    return cases


# Base images of a large-address case: BASE_IMAGES while the fp64 reference of that many images stays within twice the heaviest
# reference of the single launches above (block4's 3x3 on 64 x 64 maps, four images: 38.7 G multiply-accumulates), else 2
LARGE_REFERENCE_MACS = 2 * 38.7e9


def large_base_images(li):
    return BASE_IMAGES if BASE_IMAGES * li.flops_per_image / 2 <= LARGE_REFERENCE_MACS else 2


def large_case_id(prec, spec, n, name, kid):
    return f'{prec}:{spec_name(spec)}-b{n}:{name}:{kid}'


def _large_cases(precisions):
    scan = [c for prec in precisions for c in large_operand_scan(prec)]
    return [pytest.param(prec, spec, n, i, kid, mine, id=large_case_id(prec, spec, n, DryRun(spec, n, prec).names[i], kid))
            for prec, spec, n, i, kid, mine in large_address_cases(scan)]


def launched_large_triples(cases):
    """{triple: case id} of what the large-address cases hold, from a dry run of each case's own (precision, spec, n, layer) --
    not from what the case list says about itself: the triples with LARGE_IMAGES_BEYOND images beyond the boundary (or at the
    largest call), and those with fewer that the case names as its own."""
    out = {}
    for c in cases:
        prec, spec, n, i, kid, mine = c.values
        run = DryRun(spec, n, prec)
        assert run.kernels(n, [i]) == [kid], c.id
        now = large_triples(run.infos, i, kid, n)
        for t in held_triples(n, now) | {t for t in mine if t in now}:
            out.setdefault(t, c.id)
    return out


def test_large_operand_closure():
    """One level beside test_pair_closure: ADDRESSES.  Every other GPU case launches its large crop sides at small call sizes and
    its large call sizes at side 256 -- no operand beyond 2^32 bytes or 2^31 elements -- while the supported grid reaches
    activations of 16 GiB.  For every layer of every plan of the grid

        proc_side 64 .. 512  x  ResNet-v2 50 / 101  x  stride 4 / 8 / 16 / 32  x  h36m / many19 / merged heads  x  every batch 1 .. 256

    the size of each operand the launch touches (operand_roles: input, output, second output, residual with its own side,
    sub-sampled output, the head's fp32 logits; element sizes from the layer's dtypes) is classed A (beyond 2^31 bytes), B (beyond
    2^32 bytes), E (beyond 2^31 elements); every (kernel, role, class) triple reached -- kernel_of of
    tests/test_gpu_nonfinite_kernels.py plus the form suffix, `a & b` ids split -- must be LAUNCHED by a case of
    tests/test_gpu_large_address.py with that operand in that class and LARGE_IMAGES_BEYOND whole images beyond the boundary
    (fewer only at 256 crops, or where no call size of the grid gives them: printed).  The case list is generated from the same
    scan (large_address_cases); what the cases launch is recomputed here from each case's own dry run, so a case taken off the
    list fails this test.
    The parity modes ('f64', 'f32', 'f32m': the range of tests/test_parity_coverage.py, the same grid) reach class A too -- an
    fp64 activation is four times the fp16 one -- so their triples are part of the universe and of the list.
    Measured on the build machine: the f16 scan 2 s (47 triples, 15 cases), the three parity scans 18 s (34 triples, 10 cases);
    the whole test 30 s."""
    from tests.test_gpu_large_address import LARGE_CASES, PRECISIONS
    assert all(c.values[1] is not None for c in LARGE_CASES), LARGE_CASES[0].values[4]
    scan = [c for prec in PRECISIONS for c in large_operand_scan(prec)]
    universe = large_universe(scan)
    launched = launched_large_triples(LARGE_CASES)
    holdable = {t for c in scan for t in held_triples(c[3], c[6])}
    print(f'\n{len(universe)} (kernel, operand role, class) triples beyond 2^31 bytes over the grid, {len(LARGE_CASES)} large-address cases:')
    for c in LARGE_CASES:
        print(f'  {c.id}')
        for t, images in sorted(c.values[5].items()):
            print(f'      {t[0]}, {t[1]}, class {t[2]}: {images} images beyond' + ('' if t in holdable else '  (no call of the grid gives more)'))
    assert {'A', 'B', 'E'} <= {t[2] for t in universe} and {t[1] for t in universe} <= set(LARGE_ROLES)
    missing = sorted(t for t in universe if t not in launched)
    assert not missing, 'reached by the supported grid but launched by no large-address case (kernel, operand role, class):\n' + \
        '\n'.join(f'  {t}' for t in missing)
    # launched with the images the issue asks for: a triple some call of the grid holds is held by a case, not merely touched
    held = {t for c in LARGE_CASES for t in held_triples(c.values[2], large_triples(DryRun(c.values[1], c.values[2], c.values[0]).infos,
                                                                                   c.values[3], c.values[4], c.values[2]))}
    thin = sorted(holdable - held)
    assert not thin, f'launched with fewer than {LARGE_IMAGES_BEYOND} images beyond the boundary although the grid gives them:\n' + \
        '\n'.join(f'  {t}' for t in thin)
    # the classes are strict: a tensor of exactly 2^32 bytes / 2^31 elements (block4 at stride 4, side 256, 256 crops) is in class A only
    run = DryRun(ModelSpec(50, 4, 'h36m'))
    i = run.names.index('block4/unit_1/conv3')
    assert {t[1:] for t in large_triples(run.infos, i, run.kernels(256, [i])[0], 256)} == {('output', 'A'), ('residual', 'A')}
    assert images_beyond(68, 2 ** 26, 2 ** 32) == 4 and images_beyond(65, 2 ** 26, 2 ** 32) == 1 and images_beyond(64, 2 ** 26, 2 ** 32) == 0


def test_entries_refuse_calls_beyond_the_int32_pixel_index(lib):
    """The conv, stem and head kernels hold pixel indices in int (elements and bytes in size_t): a call whose pixel count --
    input, output, residual map, stem image, heat map -- does not fit int32 is refused with METRO_ERR_INVALID_ARG (ValueError)
    instead of launched, and nothing inside the supported grid is refused.  Through the dry run: no device, no launch."""
    one = C.c_void_p(256)                      # any non-NULL pointer: a dry run touches none
    check(lib.metro_kernel_notes(2), 'metro_kernel_notes')
    try:
        # the largest maps of the grid pass: 256 crops of side 512 (stem), their 128 x 128 maps (conv with residual, head)
        check(lib.metro_stem_pool_f32in(one, one, one, one, 256, 512, None), 'stem, grid maximum')
        d = H.conv_desc(256, 128, 512, 128, 2048, 1, residual=True, res_h=128)
        check(lib.metro_conv_f16(C.byref(d), one, one, one, None, None, one, one, None), 'conv, grid maximum')
        spec = ModelSpec(50, 4, 'h36m', proc_side=512)
        cs = spec.to_c(_lib.METRO_PREC_F16)
        check(lib.metro_head_f16(one, one, one, one, one, 256, 2048, C.byref(cs), one, None, one, None), 'head, grid maximum')
        assert lib.metro_last_kernel_id().decode().split(' & ')[:3] == ['stem_pool_f16<split2,f32in>', 'conv_pws<k512,res>', 'head_f16<144x256,k2>']
        # 2^31 pixels: 8192 crops of side 512; 131 072 maps of 128 x 128
        with pytest.raises(ValueError, match='overflow the int32 pixel index'):
            check(lib.metro_stem_pool_f32in(one, one, one, one, 8192, 512, None), 'stem')
        with pytest.raises(ValueError, match='overflow the int32 pixel index'):
            check(lib.metro_stem_pool_u8in(one, one, one, one, 8192, 512, None), 'stem')
        check(lib.metro_stem_pool_f32in(one, one, one, one, 8191, 512, None), 'stem, one crop below')
        with pytest.raises(ValueError, match='overflow the int32 pixel index'):
            check(lib.metro_head_f16(one, one, one, one, one, 131072, 2048, C.byref(cs), one, None, one, None), 'head')
        small = ModelSpec(50, 32, 'h36m')     # an 8 x 8 heat map: the pixel index fits, the grid's image axis does not
        cs2 = small.to_c(_lib.METRO_PREC_F16)
        with pytest.raises(ValueError, match='image axis'):
            check(lib.metro_head_f16(one, one, one, one, one, 65536, 2048, C.byref(cs2), one, None, one, None), 'head')
        d = H.conv_desc(131072, 128, 512, 128, 2048, 1, residual=True, res_h=128)
        with pytest.raises(ValueError, match='too many'):
            check(lib.metro_conv_f16(C.byref(d), one, one, one, None, None, one, one, None), 'conv')
        # a residual map larger than the output (the sub-sampled shortcut): its pixel count alone passes int32
        d = H.conv_desc(40000, 128, 64, 128, 256, 1, residual=True, res_h=256, res_stride=2)
        with pytest.raises(ValueError, match='too many residual pixels'):
            check(lib.metro_conv_f16(C.byref(d), one, one, one, None, None, one, one, None), 'conv, residual map')
    finally:
        lib.metro_kernel_notes(0)


def classic_dispatch_digests():
    """{spec name: sha256 over the kernel id of every layer at every call size 1 .. 256} of PAIR_SPECS' default plans, dispatched
    with the classic forms forced (metro_conv_b1_form(1))."""
    lib = _lib.load()
    runs = [DryRun(spec) for spec in PAIR_SPECS]
    out = {}
    check(lib.metro_conv_b1_form(1), 'metro_conv_b1_form')
    try:
        for run in runs:
            h = hashlib.sha256()
            for n in GRID_BATCHES:
                h.update('\0'.join(run.kernels(n)).encode() + b'\n')
            out[spec_name(run.spec)] = h.hexdigest()
    finally:
        lib.metro_conv_b1_form(0)
    return out


def test_classic_dispatch_reproduces_the_snapshot():
    """tests/golden/plan_tables_v1.json (test_plan_snapshot.py) holds the default dispatch only.  The forms behind the test switch
    metro_conv_b1_form(1) -- conv_pw64's single-role kernel in place of conv_b1_chain and conv_pws, the ring kernel's pair in
    place of block2's weight-resident one -- are what the GPU tests compare the default kernels with bit for bit, so a change of
    the dispatch must leave them where they were too.  tests/golden/classic_dispatch_v1.json was written by
    classic_dispatch_digests() from the library of the commit BEFORE the dispatch moved into csrc/conv_dispatch.cpp
    (METRO_HIP_LIB=<that library>); like the plan snapshot it is rewritten only with an intended change, from the commit before."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'classic_dispatch_v1.json')) as f:
        golden = json.load(f)
    got = classic_dispatch_digests()
    assert sorted(got) == sorted(golden)
    bad = [k for k in golden if got[k] != golden[k]]
    assert not bad, f'classic dispatch of {bad} differs from tests/golden/classic_dispatch_v1.json'


def test_every_kernel_has_a_nonfinite_case(lib):
    """Every kernel a configuration dispatches must be LAUNCHED by a case of tests/test_gpu_nonfinite_kernels.py (IEEE special
    values, store overflow and poisoned surroundings, one kernel at a time): a new kernel cannot enter the plans without one.
    A kernel is the id's family -- the text in front of '<' -- and, where one family holds several __global__ kernels with a ReLU
    of their own (head_f16: ring / 256-pixel / plain; stem_pool_f16: rows / patch), which of them (kernel_of).  What a case
    launches is taken from a dry run of its launches (metro_kernel_notes(2): nothing is launched), not from the name it states;
    and the dry run must note exactly the ids the case names."""
    from tests.test_gpu_nonfinite_kernels import NF_CASES, dry_run_ids, ids_match, kernel_of
    noted = {c.id: dry_run_ids(lib, c) for c in NF_CASES}
    wrong = {c.id: noted[c.id] for c in NF_CASES if not ids_match(noted[c.id], c.families)}
    assert not wrong, 'non-finite cases that do not reach the kernels they name:\n' + \
        '\n'.join(f'  {k}: launches {v}' for k, v in sorted(wrong.items()))
    launched = {kernel_of(k) for ids in noted.values() for k in ids}
    missing = {}
    for cname, (spec, n) in CONFIGS.items():
        for _, li, kid in dispatch_table(spec, n):
            for part in kid.split(' & '):
                if kernel_of(part) not in launched:
                    missing.setdefault(kernel_of(part), f'{cname}: {li.name.decode()} ({kid})')
    assert not missing, 'kernels without a non-finite case (first layer that dispatches each):\n' + \
        '\n'.join(f'  {k}: {w}' for k, w in sorted(missing.items()))
    # the key tells the kernels of one family apart
    assert len({kernel_of(k) for k in ('head_f16<144x256,k2>', 'head_f16<160x256>', 'head_f16<160x64>')}) == 3
    assert kernel_of('stem_pool_f16<rows,f32in>') != kernel_of('stem_pool_f16<split2,f32in>')


# the launchers that cap their grid and let a block walk several tiles (metro_common.h: note_schedule)
PERSISTENT_FAMILIES = ('conv_pw64<', 'conv_pws<', 'conv_b1_chain<', 'conv3x3_c64', 'stem_pool_f16<split')


def test_every_persistent_instantiation_has_its_schedule_cases(lib):
    """A persistent kernel keeps state from one tile to the next, so an instantiation is held not only at a shape but on every
    tile-walk schedule its predicate admits (tests/test_gpu_persistent_schedules.py: ADMITTED, CASES).  Every id of the five
    persistent families that pair_universe() or the grid of test_dispatch_closure dispatches (h36m heads: the backbones of the
    other heads are the same, which test_dispatch_closure asserts) must have a case for each class of its row: a new persistent
    instantiation cannot enter the plans without its schedules.  The rows' one shape claim -- whether the instantiation runs a
    pixel count that is no multiple of its tile -- is put to the entry points by a dry run.
    What this does and does not hold: CASES is generated from ADMITTED, so for an id that HAS a row the per-class lookup below
    cannot fail; the live parts are the missing row (a new id), the ragged flag, and that the stem and conv_b1_chain rows are
    the full lists of the module.  Whether a row names every schedule its kernel has is a matter of review, not of this test."""
    from tests import test_gpu_persistent_schedules as PS
    ids = {part for kid, _ in pair_universe() for part in kid.split(' & ')}
    for side in GRID_SIDES:
        for arch in GRID_ARCHS:
            for stride in GRID_STRIDES:
                run = DryRun(ModelSpec(arch, stride, 'h36m', proc_side=side))
                layers = [i for i, name in enumerate(run.names) if name not in ('logits', 'softargmax')]
                for n in GRID_BATCHES:
                    ids.update(part for kid in run.kernels(n, layers) for part in kid.split(' & '))
    persistent = sorted(k for k in ids if k.startswith(PERSISTENT_FAMILIES))
    assert len(persistent) >= 15, persistent
    have = {(inst.kid, cls) for inst, cls in PS.CASES}
    missing = [(k, cls) for k in persistent for cls in PS.ADMITTED.get(k, ('<no row in ADMITTED>',)) if (k, cls) not in have]
    assert not missing, 'persistent instantiations dispatched by the plans without a schedule case:\n' + '\n'.join(f'  {k}: {c}' for k, c in missing)
    full = {'pw64': PS.STRIDED, 'pws': PS.STRIDED, 'b1': PS.NO_MAP, 'c64': PS.C64_CLASSES, 'stem': PS.STEM_CLASSES}
    for inst in PS.INSTANCES:           # no row is trimmed: the family's whole list, the four sub-sampled variants for `two-three`
        want = set(full[inst.family])
        if 'subout' in inst.kid:
            want = want - {'two-three'} | set(PS.SUBOUT)
        assert set(PS.ADMITTED[inst.kid]) - {'ragged-late'} == want, inst.kid
    for inst in PS.INSTANCES:
        if inst.family in ('c64', 'stem'):
            assert 'ragged-late' not in PS.ADMITTED[inst.kid]          # whole tiles by construction (map rows, patches)
            continue
        try:
            (noted, _), _ = PS.dry_run(lib, inst, 'ragged-late', 256)
        except ValueError:                                             # the entry refuses the shape
            noted = []
        assert (tuple(noted) == inst.before + (inst.kid,)) == ('ragged-late' in PS.ADMITTED[inst.kid]), (inst.kid, noted)


@pytest.mark.parametrize('nb', [3, 8], ids=['64-pixel-tiles', '256-pixel-tiles'])
def test_head_partials_slot_covers_large_heat_maps(lib, nb):
    """The one-launch head writes one fp32 record per (image, slab, joint): one per 64 pixels, and one per 32 pixels once the
    launch has >= 256 tiles of 256 pixels (head_f16<160x256>) -- more slabs than the two-launch path's cap of 64 once the heat
    map has > 4096 pixels (proc_side 384 at stride 4 = 96 x 96).  The partials slot (followed only by the 4-byte-per-image
    status words) must hold what the library itself says a launch at this batch writes."""
    spec = ModelSpec(50, 4, 'h36m', proc_side=384)
    eng = Engine(spec, None, 'f16', max_batch=nb)
    infos = eng.layer_infos()
    logits = next(li for li in infos if li.name == b'logits')
    kern = eng.layer_kernels(nb)[infos.index(logits)]
    assert kern == 'head_f16<144x256,k2>' if nb == 8 else kern.startswith('head_f16<') and 'x256' not in kern, kern
    side, j = 96, spec.skeleton.n_head
    after_logits = logits.out_offset + logits.out_bytes_per_image * nb
    need = lib.metro_head_f16_scratch_bytes(nb, side, j)
    assert need >= nb * (side * side // 32) * j * 5 * 4          # a record per 32 pixels
    status = -(-nb * 4 // 256) * 256
    assert eng.workspace_bytes - after_logits - status >= need, (eng.workspace_bytes - after_logits - status, need)


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def _assignment(n, what):
    """Which of the min(BASE_IMAGES, n) base images each position of the batch holds (H.crop_assignment), seeded by the case."""
    return H.crop_assignment(n, min(BASE_IMAGES, n), zlib.crc32(what.encode()))


def _base_images(assign):
    """p of an assignment: every base image occurs (min(BASE_IMAGES, n) for _assignment's; a large-address case may use 2)."""
    return int(np.max(assign)) + 1


def _twins(gen, assign, shape, cuda, scale=1.0, relu=False):
    """fp16 [n, *shape] on the device with image i == base image assign[i], and the base images as numpy."""
    p = _base_images(assign)
    base = torch.randn((p,) + tuple(shape), generator=gen, device=cuda, dtype=torch.float32) * scale
    if relu:
        base = base.clamp_min(0)
    base = base.half()
    return H.lay_out_twins(base, assign), base.cpu().numpy()


def _noted(lib):
    return lib.metro_last_kernel_id().decode().split(' & ')


def _close(got, ref, what, tol=2e-3):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), what
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    print(f'\n[{what}] worst |d| / layer maximum {err / scale:.2e} (bar {tol:g})')
    assert err <= tol * scale, (what, err, scale)


@pytest.mark.gpu
@pytest.mark.parametrize('cname,layer,kid', _CASES)
def test_production_dispatch_against_fp64_reference(lib, cuda, cname, layer, kid):
    assert cname is not None, f'libmetro_hip.so could not be loaded at collection time: {kid}'
    spec, n = CONFIGS[cname]
    if dispatch_table(spec, n)[layer][1].name == b'softargmax' and kid == 'softargmax_finalize<acc32>':
        pytest.skip('launched (and compared) together with the head: see the logits case of this configuration')
    _launch(lib, cuda, cname, spec, n, layer, kid)


@pytest.mark.gpu
@pytest.mark.parametrize('spec,n,layer,kid', _SINGLE_CASES)
def test_single_launch_against_fp64_reference(lib, cuda, spec, n, layer, kid):
    """SINGLE_LAUNCHES and the (kernel id, layer shape) pairs of test_pair_closure that no other case launches: one launch each,
    at the smallest call that brings the instantiation to that layer shape, held like the configurations' cases -- the entry
    point launches what the plan names, fp64 reference on the same fp16 operands (2e-3 of the layer maximum for fp16 outputs,
    2e-5 for fp32 ones, 2e-3 mm for poses), every position of the call carrying its twin's bits."""
    assert spec is not None, f'libmetro_hip.so could not be loaded at collection time: {kid}'
    _launch(lib, cuda, f'{spec_name(spec)}-b{n}', spec, n, layer, kid)


def _launch(lib, cuda, cname, spec, n, layer, kid, assign=None):
    """One launch of `layer` of the f16 plan of `spec` at call size n through its single-kernel entry point, held to the id the
    plan names, to the twin layout and to the fp64 reference on the base images.  `assign`: the layout (default: _assignment)."""
    _, li, kid2 = dispatch_table(spec, n)[layer]
    assert kid2 == kid
    name = li.name.decode()
    gen = torch.Generator(device=cuda)
    gen.manual_seed(zlib.crc32(f'{cname}/{name}'.encode()))
    rng = np.random.default_rng(zlib.crc32(f'{cname}/{name}/w'.encode()))
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dt))).to(cuda)
    if assign is None:
        assign = _assignment(n, f'{cname}/{name}')
    assert len(assign) == n
    check(lib.metro_kernel_notes(1), 'metro_kernel_notes')
    try:
        if name == 'softargmax':
            _softargmax(lib, cuda, spec, assign, gen, rng, kid)
        elif name == 'conv1+pool1':
            _stem(lib, cuda, li, assign, gen, rng, dev, kid)
        elif name == 'logits' and kid.startswith('head_f16'):
            _head(lib, cuda, spec, li, assign, gen, rng, dev, kid)
        else:
            _conv(lib, cuda, li, assign, gen, rng, dev, kid, name)
    finally:
        lib.metro_kernel_notes(0)


def _stem(lib, cuda, li, assign, gen, rng, dev, kid):
    side = 4 * li.h_out
    n = len(assign)
    p = _base_images(assign)
    base = torch.rand((p, side, side, 3), generator=gen, device=cuda, dtype=torch.float32)
    img = H.lay_out_twins(base, assign)
    w = (rng.standard_normal((64, 7, 7, 3)) * np.sqrt(2.0 / 147)).astype(np.float16)
    b = (rng.standard_normal(64) * 0.5).astype(np.float32)
    wp = np.zeros((64, 7, 8, 4), np.float16)
    wp[:, :, :7, :3] = w
    tw, tb = dev(wp, np.float16), dev(b, np.float32)
    out = torch.full((n, side // 4, side // 4, 64), float('nan'), dtype=torch.float16, device=cuda)
    check(lib.metro_stem_pool_f32in(H.ptr(img), H.ptr(tw), H.ptr(tb), H.ptr(out), n, side, None), 'metro_stem_pool_f32in')
    torch.cuda.synchronize()
    assert _noted(lib) == [kid], (_noted(lib), kid)
    H.assert_twins(out, assign, p, kid)
    xi = torch.from_numpy(base.cpu().numpy().astype(np.float16).astype(np.float64)).permute(0, 3, 1, 2)
    conv = torch.nn.functional.conv2d(torch.nn.functional.pad(xi, (3, 3, 3, 3)), torch.from_numpy(w.astype(np.float64)).permute(0, 3, 1, 2),
                                      torch.from_numpy(b.astype(np.float64)), stride=2).half().double()
    want = torch.nn.functional.max_pool2d(torch.nn.functional.pad(conv, (1, 1, 1, 1)), 3, 2).permute(0, 2, 3, 1).numpy()
    _close(out[:p].cpu().numpy(), want, kid)


def _head(lib, cuda, spec, li, assign, gen, rng, dev, kid):
    from oracle.forward import logits_to_output
    side, k, c = li.h_in, li.c_in, li.c_out
    n = len(assign)
    x, xb = _twins(gen, assign, (side, side, k), cuda)
    w = (rng.standard_normal((c, k)) * np.sqrt(2.0 / k) * 2.0).astype(np.float16)
    b = (rng.standard_normal(c) * 0.1).astype(np.float32)
    sc = rng.uniform(0.5, 1.5, k).astype(np.float16)
    sh = (rng.standard_normal(k) * 0.2).astype(np.float16)
    tw, tb, ts, tsh = dev(w, np.float16), dev(b, np.float32), dev(sc, np.float16), dev(sh, np.float16)
    cs = spec.to_c(_lib.METRO_PREC_F16)
    scratch = torch.empty(lib.metro_head_f16_scratch_bytes(n, side, spec.skeleton.n_head), dtype=torch.uint8, device=cuda)
    logits = torch.full((n, side, side, c), float('nan'), dtype=torch.float32, device=cuda)
    poses = torch.full((n, spec.skeleton.n_out, 3), float('nan'), dtype=torch.float32, device=cuda)
    check(lib.metro_head_f16(H.ptr(x), H.ptr(tw), H.ptr(tb), H.ptr(ts), H.ptr(tsh), n, k, C.byref(cs), H.ptr(scratch), H.ptr(logits),
                             H.ptr(poses), None), 'metro_head_f16')
    torch.cuda.synchronize()
    assert _noted(lib) == [kid, 'softargmax_finalize<acc32>'], _noted(lib)
    p = xb.shape[0]
    H.assert_twins(logits, assign, p, kid)
    H.assert_twins(poses, assign, p, kid + ' (poses)')
    xin = np.maximum((xb.astype(np.float64) * sc.astype(np.float64) + sh.astype(np.float64)).astype(np.float16).astype(np.float64), 0)
    ref = xin.reshape(-1, k) @ w.astype(np.float64).T + b.astype(np.float64)
    ref = ref.reshape(p, side, side, c)
    got = logits[:p].cpu().double().numpy()
    want = logits_to_output(H.oracle_spec(spec), ref).numpy()
    d = np.abs(poses[:p].cpu().numpy() - want).max()
    print(f'\n[{kid}] logits: worst |d| / maximum {np.abs(got - ref).max() / np.abs(ref).max():.2e} (bar 2e-05); poses {d:.2e} mm (bar 0.002)')
    assert np.abs(got - ref).max() <= 2e-5 * np.abs(ref).max(), np.abs(got - ref).max() / np.abs(ref).max()
    assert d <= 2e-3, f'{kid}: poses {d} mm from the exact soft-argmax of the exact logits'


def _softargmax(lib, cuda, spec, assign, gen, rng, kid):
    """The two-launch soft-argmax behind a head that is not whole tiles, on fp32 logits at the layer's real side and batch:
    N(0, 4) plus one planted peak per (image, joint) at a random voxel, so no pose is the map centre."""
    from oracle.forward import logits_to_output
    side, j, dd = spec.heatmap_side, spec.skeleton.n_head, spec.depth
    n = len(assign)
    p = _base_images(assign)
    base = torch.randn((p, side, side, dd * j), generator=gen, device=cuda, dtype=torch.float32) * 4.0
    for i in range(p):
        for jj in range(j):
            h, w, d = (int(v) for v in rng.integers(0, (side, side, dd)))
            base[i, h, w, d * j + jj] += 12.0
    logits = H.lay_out_twins(base, assign)
    cs = spec.to_c(_lib.METRO_PREC_F16)
    scratch = torch.empty(lib.metro_softargmax_scratch_bytes(n, side, j), dtype=torch.uint8, device=cuda)
    poses = torch.full((n, spec.skeleton.n_out, 3), float('nan'), dtype=torch.float32, device=cuda)
    check(lib.metro_softargmax(H.ptr(logits), n, C.byref(cs), _lib.METRO_PREC_F16, H.ptr(scratch), H.ptr(poses), None), 'metro_softargmax')
    torch.cuda.synchronize()
    assert _noted(lib) == kid.split(' & '), f'the entry point launched {_noted(lib)}, the plan names {kid}'
    H.assert_twins(poses, assign, p, kid)
    want = logits_to_output(H.oracle_spec(spec), base.cpu().double().numpy()).numpy()
    got = poses[:p].cpu().numpy()
    assert np.isfinite(got).all(), kid
    d = np.abs(got - want).max()
    print(f'\n[{kid}] poses {d:.2e} mm (bar 0.002)')
    assert d <= 2e-3, f'{kid}: poses {d} mm from the exact soft-argmax of the same logits'
    # the planted peaks pull the joints off the centre: the comparison is not of two maps' centres
    assert np.abs(want).max() > 50.0, np.abs(want).max()


def _conv(lib, cuda, li, assign, gen, rng, dev, kid, name):
    n = len(assign)
    pair = name.endswith('/shortcut+conv1')
    nxt = '/conv3+' in name
    c_in, c1 = li.c_in, li.c_out
    c_out = c1 + li.out2_channels if pair else c1
    k, h_in, h_out = li.kh, li.h_in, li.h_out
    assert li.kh == li.kw and li.h_in == li.w_in and li.pad_top == li.pad_left
    f32out = li.out_dtype == _lib.METRO_F32
    rebuilt = bool(li.fused_flags & _lib.FUSED_REBUILT_SHORTCUT)      # the shortcut is rebuilt in the launch: no residual tensor
    compact = bool(li.fused_flags & _lib.FUSED_COMPACT_SHORTCUT)      # the sub-sampled shortcut arrives as a compact tensor
    has_res = bool(li.has_residual) and not rebuilt
    res_stride, res_offset = (1, 0) if compact else (li.res_stride, li.res_offset)
    res_h = h_out if res_stride == 1 else 2 * h_out
    d = H.conv_desc(n, h_in, c_in, h_out, c_out, k, li.stride, li.dilation, li.pad_top, prologue=bool(li.has_prologue),
                    relu=bool(li.relu), residual=has_res, res_h=res_h, res_stride=res_stride,
                    res_offset=res_offset, out_dtype=_lib.METRO_F32 if f32out else _lib.METRO_F16, in_dtype=_lib.METRO_F16)
    x, xb = _twins(gen, assign, (h_in, h_in, c_in), cuda, relu=not li.has_prologue and k == 3)
    w = (rng.standard_normal((c_out, k, k, c_in)) * np.sqrt(2.0 / (k * k * c_in))).astype(np.float16)
    b = (rng.standard_normal(c_out) * 0.1).astype(np.float32)
    tw, tb = dev(w, np.float16), dev(b, np.float32)
    ts = tsh = tr = None
    pro = None
    if li.has_prologue:
        pro = (rng.uniform(0.5, 1.5, c_in).astype(np.float16), (rng.standard_normal(c_in) * 0.2).astype(np.float16))
        ts, tsh = dev(pro[0], np.float16), dev(pro[1], np.float16)
    rb = None
    if has_res:
        tr, rb = _twins(gen, assign, (res_h, res_h, c_out), cuda)
    out = torch.full((n, h_out, h_out, c1), float('nan'), dtype=torch.float32 if f32out else torch.float16, device=cuda)
    out2 = None
    if li.fused_flags & _lib.FUSED_CONV1_IN_FRONT:
        return _conv1_conv2(lib, cuda, li, assign, d, x, xb, tw, tb, w, b, out, rng, dev, kid)
    psc = None
    if li.fused_flags & (_lib.FUSED_PROJECTION_SHORTCUT | _lib.FUSED_REBUILT_SHORTCUT):
        assert nxt, 'the in-launch projection shortcut exists in the conv3 + next conv1 launch only'
        cx = 64                                   # the unit's raw input (block1/unit_1: the pooled stem output)
        xs, xsb = _twins(gen, assign, (h_out, h_out, cx), cuda)
        wsc = (rng.standard_normal((c1, cx)) * np.sqrt(2.0 / cx)).astype(np.float16)
        bsc = (rng.standard_normal(c1) * 0.1).astype(np.float32)
        psc_s = rng.uniform(0.5, 1.5, cx).astype(np.float16)
        psc_b = (rng.standard_normal(cx) * 0.2).astype(np.float16)
        psc = [xs, dev(wsc, np.float16), dev(bsc, np.float32), dev(psc_s, np.float16), dev(psc_b, np.float16)]
    if pair:
        out2 = torch.full((n, h_out, h_out, li.out2_channels), float('nan'), dtype=torch.float16, device=cuda)
        check(lib.metro_conv_f16_pair(C.byref(d), H.ptr(x), H.ptr(tw), H.ptr(tb), H.ptr(ts), H.ptr(tsh), H.ptr(out), c1, H.ptr(out2), None),
              'metro_conv_f16_pair')
        if kid.startswith('conv_pw64<k256'):   # block2's pair in the weight-resident kernel and in the ring kernel it replaced: the same bits
            torch.cuda.synchronize()
            mine, mine2 = out.clone(), out2.clone()
            check(lib.metro_conv_b1_form(1), 'metro_conv_b1_form')
            try:
                check(lib.metro_conv_f16_pair(C.byref(d), H.ptr(x), H.ptr(tw), H.ptr(tb), H.ptr(ts), H.ptr(tsh), H.ptr(out), c1, H.ptr(out2), None),
                      'metro_conv_f16_pair (ring kernel)')
                torch.cuda.synchronize()
            finally:
                lib.metro_conv_b1_form(0)
            assert _noted(lib)[-1].startswith('conv_igemm_f16_dma<'), _noted(lib)
            assert torch.equal(out, mine) and torch.equal(out2, mine2), f'{kid}: differs from {_noted(lib)[-1]}'
            check(lib.metro_kernel_notes(1), 'metro_kernel_notes')
            check(lib.metro_conv_f16_pair(C.byref(d), H.ptr(x), H.ptr(tw), H.ptr(tb), H.ptr(ts), H.ptr(tsh), H.ptr(out), c1, H.ptr(out2), None),
                  'metro_conv_f16_pair')
    elif nxt:
        c2 = li.out2_channels
        w2 = (rng.standard_normal((c2, c1)) * np.sqrt(2.0 / c1)).astype(np.float16)
        b2 = (rng.standard_normal(c2) * 0.1).astype(np.float32)
        sc2 = rng.uniform(0.5, 1.5, c1).astype(np.float16)
        sh2 = (rng.standard_normal(c1) * 0.2).astype(np.float16)
        t2 = [dev(w2, np.float16), dev(b2, np.float32), dev(sc2, np.float16), dev(sh2, np.float16)]
        out2 = torch.full((n, h_out, h_out, c2), float('nan'), dtype=torch.float16, device=cuda)
        on_chip = bool(li.fused_flags & _lib.FUSED_OUT_ON_CHIP)
        prev = None
        if rebuilt:
            # block1/unit_2: x_1 = fp16(W3_prev . t2_prev + b) + fp16(Wsc . pre(x0) + bsc) is rebuilt in the launch.  The storing form
            # (what metro_forward_upto runs) gives `out`; the form the plan names must give the SAME second output, and its
            # sub-sampled copy must be those pixels of `out`
            tp, tpb = _twins(gen, assign, (h_out, h_out, 64), cuda, relu=True)
            w3p = (rng.standard_normal((c1, 64)) * np.sqrt(2.0 / 64)).astype(np.float16)
            b3p = (rng.standard_normal(c1) * 0.1).astype(np.float32)
            prev = [tp, dev(w3p, np.float16), dev(b3p, np.float32)]
            args = lambda o, osub, soff, o2: (C.byref(d), H.ptr(x), H.ptr(tw), H.ptr(tb), H.ptr(psc[0]), H.ptr(psc[1]), H.ptr(psc[2]), H.ptr(psc[3]),
                                              H.ptr(psc[4]), H.ptr(prev[0]), H.ptr(prev[1]), H.ptr(prev[2]), H.ptr(o), H.ptr(osub), soff, H.ptr(t2[0]),
                                              H.ptr(t2[1]), H.ptr(t2[2]), H.ptr(t2[3]), H.ptr(o2), c2, None)
            # the classic single-role kernel first (what metro_forward_upto runs: the whole sum stored) ...
            check(lib.metro_conv_b1_form(1), 'metro_conv_b1_form')
            try:
                check(lib.metro_conv_f16_next_rebuild(*args(out, None, 0, out2)), 'metro_conv_f16_next_rebuild (classic form)')
                torch.cuda.synchronize()
            finally:
                lib.metro_conv_b1_form(0)
            full, full2 = out.clone(), out2.clone()
            # ... then the form the plan names: same sum (or exactly its sub-sampled pixels), same second output, bit for bit
            check(lib.metro_kernel_notes(1), 'metro_kernel_notes')
            out.fill_(float('nan'))
            out2.fill_(float('nan'))
            if li.out_sub_offset >= 0:
                sub = torch.full((n, li.out_sub_side, li.out_sub_side, c1), float('nan'), dtype=torch.float16, device=cuda)
                check(lib.metro_conv_f16_next_rebuild(*args(None, sub, li.out_sub_off, out2)), 'metro_conv_f16_next_rebuild')
                torch.cuda.synchronize()
                o = li.out_sub_off
                assert torch.equal(sub, full[:, o::2, o::2][:, :li.out_sub_side, :li.out_sub_side]), f'{kid}: sub-sampled copy != pixels of the classic form\'s sum'
                out.copy_(full)
            else:
                check(lib.metro_conv_f16_next_rebuild(*args(out, None, 0, out2)), 'metro_conv_f16_next_rebuild')
                torch.cuda.synchronize()
                assert torch.equal(out, full), f'{kid}: the sum differs between the classic and the producer / consumer form'
            assert torch.equal(out2, full2), f'{kid}: second output differs between the classic and the producer / consumer form'
        elif psc is not None:
            pargs = lambda o, o2: (C.byref(d), H.ptr(x), H.ptr(tw), H.ptr(tb), H.ptr(psc[0]), H.ptr(psc[1]), H.ptr(psc[2]), H.ptr(psc[3]), H.ptr(psc[4]),
                                   H.ptr(o), H.ptr(t2[0]), H.ptr(t2[1]), H.ptr(t2[2]), H.ptr(t2[3]), H.ptr(o2), c2, None)
            if on_chip:           # the plan's form keeps the sum on chip: same second output as the classic storing form
                check(lib.metro_conv_b1_form(1), 'metro_conv_b1_form')
                try:
                    check(lib.metro_conv_f16_next_proj(*pargs(out, out2)), 'metro_conv_f16_next_proj (classic form)')
                    torch.cuda.synchronize()
                finally:
                    lib.metro_conv_b1_form(0)
                full2 = out2.clone()
                check(lib.metro_kernel_notes(1), 'metro_kernel_notes')
                out2.fill_(float('nan'))
                check(lib.metro_conv_f16_next_proj(*pargs(None, out2)), 'metro_conv_f16_next_proj (sum on chip)')
                torch.cuda.synchronize()
                assert torch.equal(out2, full2), f'{kid}: second output differs between the classic storing and the on-chip form'
            else:
                check(lib.metro_conv_f16_next_proj(*pargs(out, out2)), 'metro_conv_f16_next_proj')
        else:
            check(lib.metro_conv_f16_next(C.byref(d), H.ptr(x), H.ptr(tw), H.ptr(tb), H.ptr(tr), H.ptr(out), H.ptr(t2[0]), H.ptr(t2[1]),
                                          H.ptr(t2[2]), H.ptr(t2[3]), H.ptr(out2), c2, None), 'metro_conv_f16_next')
    else:
        check(lib.metro_conv_f16(C.byref(d), H.ptr(x), H.ptr(tw), H.ptr(tb), H.ptr(ts), H.ptr(tsh), H.ptr(tr), H.ptr(out), None),
              'metro_conv_f16')
        if kid.endswith('+subgrid'):
            # the tap-reuse kernel in sub-grid pixel order against the ring kernel these layers ran on until round 6 (the test
            # switch puts them back): two correct fp32 summation orders of the same products (chunk-major vs tap-major) --
            # rounding flips of the fp16 result only

            torch.cuda.synchronize()
            sub = out.clone()
            check(lib.metro_conv_b1_form(1), 'metro_conv_b1_form')
            try:
                check(lib.metro_conv_f16(C.byref(d), H.ptr(x), H.ptr(tw), H.ptr(tb), H.ptr(ts), H.ptr(tsh), H.ptr(tr), H.ptr(out), None),
                      'metro_conv_f16 (classic form)')
                torch.cuda.synchronize()
            finally:
                lib.metro_conv_b1_form(0)
            assert _noted(lib)[-1].startswith('conv_igemm_f16_dma<'), _noted(lib)
            same = (out == sub).float().mean().item()
            worst = (out.float() - sub.float()).abs().max().item()
            assert same >= 0.97 and worst <= 2.0 ** -9 * sub.float().abs().max().item(), (kid, same, worst)
            check(lib.metro_kernel_notes(1), 'metro_kernel_notes')
            check(lib.metro_conv_f16(C.byref(d), H.ptr(x), H.ptr(tw), H.ptr(tb), H.ptr(ts), H.ptr(tsh), H.ptr(tr), H.ptr(out), None), 'metro_conv_f16')
        if kid.startswith('conv_pws<'):        # the skewed kernel and conv_pw64's lock-step one: the same bits
            torch.cuda.synchronize()
            skewed = out.clone()
            noted = _noted(lib)
            check(lib.metro_conv_b1_form(1), 'metro_conv_b1_form')
            try:
                check(lib.metro_conv_f16(C.byref(d), H.ptr(x), H.ptr(tw), H.ptr(tb), H.ptr(ts), H.ptr(tsh), H.ptr(tr), H.ptr(out), None),
                      'metro_conv_f16 (classic form)')
                torch.cuda.synchronize()
            finally:
                lib.metro_conv_b1_form(0)
            assert _noted(lib)[-1].startswith('conv_pw64<'), _noted(lib)
            assert torch.equal(out, skewed), f'{kid}: differs from {_noted(lib)[-1]}'
            check(lib.metro_kernel_notes(1), 'metro_kernel_notes')
            check(lib.metro_conv_f16(C.byref(d), H.ptr(x), H.ptr(tw), H.ptr(tb), H.ptr(ts), H.ptr(tsh), H.ptr(tr), H.ptr(out), None), 'metro_conv_f16')
    torch.cuda.synchronize()
    assert _noted(lib) == kid.split(' & '), f'the entry point launched {_noted(lib)}, the plan names {kid}'     # (a layer may be two launches)
    p = xb.shape[0]
    H.assert_twins(out, assign, p, kid)
    if out2 is not None:
        H.assert_twins(out2, assign, p, kid + ' (second output)')
    xin = xb.astype(np.float64)
    if pro is not None:       # fp16 FMA + ReLU, one rounding (v_pk_fma_f16)
        xin = np.maximum((xin * pro[0].astype(np.float64) + pro[1].astype(np.float64)).astype(np.float16).astype(np.float64), 0)
    ref = H.ref_conv_nhwc(xin, w, b, li.stride, li.dilation, li.pad_top, h_out, relu=bool(li.relu) and not pair).numpy()
    got = out[:p].cpu().double().numpy()
    if pair:
        _close(got, ref[..., :c1], kid)
        _close(out2[:p].cpu().numpy(), np.maximum(ref[..., c1:], 0), kid + ' (second output)')
        return
    if rb is not None:        # fp16(conv + bias), then the fp16 Add of the (sub-sampled, shifted) shortcut
        r = rb.astype(np.float64)[:, res_offset::res_stride, res_offset::res_stride][:, :h_out, :h_out]
        ref = ref.astype(np.float16).astype(np.float64) + r
    if psc is not None:       # fp16(conv3 + bias) + fp16(Wsc . fp16(relu(x * s + b)) + bias_sc): the fp16 Add of resnet_v2.py:138
        xin_s = np.maximum((xsb.astype(np.float64) * psc_s.astype(np.float64) + psc_b.astype(np.float64)).astype(np.float16).astype(np.float64), 0)
        sc = (xin_s @ wsc.astype(np.float64).T + bsc.astype(np.float64)).astype(np.float16).astype(np.float64)
        if rebuilt:           # x_1 = fp16(fp16(W3_prev . t2_prev + b) + projection shortcut), then THIS unit's fp16 Add
            c3p = (tpb.astype(np.float64) @ w3p.astype(np.float64).T + b3p.astype(np.float64)).astype(np.float16).astype(np.float64)
            sc = (c3p + sc).astype(np.float16).astype(np.float64)
        ref = ref.astype(np.float16).astype(np.float64) + sc
    _close(got, ref, kid, tol=2e-5 if f32out else 2e-3)
    if nxt:
        pre = np.maximum((got * sc2.astype(np.float64) + sh2.astype(np.float64)).astype(np.float16).astype(np.float64), 0)
        want2 = np.maximum(pre @ w2.astype(np.float64).T + b2.astype(np.float64), 0)
        _close(out2[:p].cpu().numpy(), want2, kid + ' (second output)')


def _conv1_conv2(lib, cuda, li, assign, d, x, xb, tw2, tb2, w2, b2, out, rng, dev, kid):
    """conv1 (1x1 on the pre-activated input, folded BN + ReLU) fused in front of the 3x3: t1 is rounded to fp16 once (in LDS)."""
    c = li.c_in
    w1 = (rng.standard_normal((li.c_out, c)) * np.sqrt(2.0 / c)).astype(np.float16)
    b1 = (rng.standard_normal(li.c_out) * 0.1).astype(np.float32)
    ps = rng.uniform(0.5, 1.5, c).astype(np.float16)
    pb = (rng.standard_normal(c) * 0.2).astype(np.float16)
    t = [dev(w1, np.float16), dev(b1, np.float32), dev(ps, np.float16), dev(pb, np.float16)]
    check(lib.metro_conv_f16_conv1_conv2(C.byref(d), H.ptr(x), H.ptr(t[0]), H.ptr(t[1]), H.ptr(t[2]), H.ptr(t[3]), H.ptr(tw2), H.ptr(tb2),
                                         H.ptr(out), None), 'metro_conv_f16_conv1_conv2')
    torch.cuda.synchronize()
    assert _noted(lib) == kid.split(' & '), f'the entry point launched {_noted(lib)}, the plan names {kid}'     # (a layer may be two launches)
    H.assert_twins(out, assign, xb.shape[0], kid)
    xin = np.maximum((xb.astype(np.float64) * ps.astype(np.float64) + pb.astype(np.float64)).astype(np.float16).astype(np.float64), 0)
    t1 = np.maximum(xin @ w1.astype(np.float64).T + b1.astype(np.float64), 0).astype(np.float16)
    ref = H.ref_conv_nhwc(t1, w2, b2, 1, 1, 1, li.h_out, relu=True).numpy()
    _close(out[:xb.shape[0]].cpu().numpy(), ref, kid)
