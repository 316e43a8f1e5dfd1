"""The BENCHMARKED fp16 path, layer by layer at full width, against the fp16-faithful oracle (`-m gpu`).

oracle/f16emu.py restates the graph with one fp16 rounding per stored tensor (the arithmetic the f16 mode of the
HIP path implements; see its header for how that relates to the reference's fp16 graph).  What is left between
the two is the accumulation order inside a convolution (fp32 MFMA vs exact): one-ulp flips of fp16 results.

Two comparisons, over EVERY launch of the plan and both outputs of fused launches:

  * per launch ("teacher forced"): the oracle function of that tensor is fed the HIP path's OWN input tensors, so
    nothing propagates and the bar is a rounding flip: every element within ONE fp16 ulp of its own magnitude
    (floored at 1/64 of the layer maximum, where the absolute fp32 accumulation noise of a dot product lives) and
    >= 99 % of the elements bit-identical.  A wrong tile, channel, tap, pad or residual cannot pass this.
  * whole graph: one-ulp flips of a large activation move every output of that pixel by w * ulp, so two fp16
    chains decorrelate at the ulp level with depth (measured: 99.96 % identical after the stem, ~20-60 % in
    block4, poses 0.3-2 mm apart -- the same distance either chain has to exact math).  The layers are held to
    8 ulps of the layer maximum end to end; the POSES must be as close to the exact (fp64) oracle as the fp16
    oracle's own poses are (mean x 2, max x 2.5): fp16 storage costs 1.5-3.5 mm on these nets, and the HIP
    path may not cost more.  The soft-argmax launch is held to 1e-3 mm against exact math on its own fp32 logits.

Real-batch cases ({'batch': N}): the dispatch depends on the batch, so the call has N crops -- built from the case's few oracle
crops by H.crop_assignment, a layout without period or repeated aligned group (tests/test_crop_assignment.py).  The oracle
comparisons above run on positions 0 .. crops - 1; every position of every tensor (both outputs of fused launches, the poses)
must carry the bits of its twin (H.assert_twins, on the device), so a launch that is right on the first crops and misplaces
or damages a tile in the middle of the call fails.  Measured on an MI355X for the cases at the production batches (teacher
forced: worst element in ulps of its own magnitude / least share of bit-identical elements, and its layer; whole graph: worst
layer in ulps of the layer maximum; poses against exact math, and the fp16 model's own distance):

    rn101-s8-many19-n2-of-batch32 (C4)    1.00 / 99.892 % (block4/unit_1/shortcut+conv1)   5.50 (block3/unit_21/conv2)   2.845 mm (model 2.669)
    rn50-s4-h36m-n2-of-batch16 (C5)       1.00 / 99.889 % (block4/unit_1/shortcut+conv1)   4.00 (block3/unit_4/conv3)    2.485 mm (model 2.560)
    rn50-s32-h36m-n2-side224-of-batch64   1.00 / 99.878 % (block4/unit_1/conv2)            3.31 (block3/unit_4/conv1)    2.263 mm (model 2.427)
    rn50-s8-h36m-n2-of-batch32            1.00 / 99.888 % (block4/unit_1/shortcut+conv1)   4.00 (block3/unit_5/conv3)    1.460 mm (model 1.846)
    the ragged calls (no exact-math run):
    rn50-s16-h36m-n2-of-batch13           1.00 / 99.893 % (block4/unit_1/shortcut+conv1)   4.00 (block3/unit_6/conv3)    soft-argmax 3.3e-4 mm
    rn50-s32-h36m-n2-of-batch63           1.00 / 99.887 % (block4/unit_3/conv2)            4.00 (block3/unit_6/conv3)    soft-argmax 2.8e-4 mm
    rn101-s8-many19-n2-of-batch13         1.00 / 99.892 % (block4/unit_1/shortcut+conv1)   5.50 (block3/unit_23/conv3)   soft-argmax 4.0e-4 mm
    rn50-s4-h36m-n2-of-batch5             1.00 / 99.888 % (block4/unit_1/shortcut+conv1)   4.00 (block3/unit_6/conv3)    soft-argmax 3.0e-4 mm

(the one-ulp figure is the stem's in every case; soft-argmax 2.7e-4 to 3.6e-4 mm; no twin differs anywhere).  The pose distances
of the first, second and fourth were measured once with the exact-math run that these cases no longer make ('pose_ratios': False,
see CASES): for C4 and C5 at these batches the pose criterion is test_gpu_forward.py::test_batch_independence_of_the_other_
baseline_configs's; for stride 8 with 17 joints the layer bars and the soft-argmax bar are what holds the poses at 32 crops.
"""
import os
import zlib

import numpy as np
import pytest
import torch

from metro_pose3d_amd import ModelSpec, _lib, synth
from metro_pose3d_amd.engine import Engine
from oracle import f16emu
from oracle import forward as OF
from oracle.forward import coords01_to_output, soft_argmax01
from oracle.spec import head_joint_info, schedule
from tests import helpers as H

pytestmark = pytest.mark.gpu

POSE_RATIO = 2.0               # whole graph: mean |hip - exact| <= POSE_RATIO * mean |fp16 oracle - exact|.  Two fp16 realisations are two
                               # draws of the same rounding noise and a crop has 51-57 strongly correlated values: the ratio moves
                               # with every change of a summation order (0.9-1.6 observed over the cases and kernel versions)
POSE_RATIO_MAX = 2.5           # ... and the maximum (of 17-57 values per crop: a noisy statistic) within this factor
SOFTARGMAX_TOL_MM = 1e-3       # soft-argmax kernel (fp32, fast exp) vs exact math on the same fp32 logits
CHAIN_ULPS_OF_MAX = 8.0        # whole-graph layer tensors, in fp16 ulps of the layer maximum
MIN_IDENTICAL = 0.995          # same-input comparison: fraction of bit-identical elements per tensor


def ospec_joints(ospec):
    return head_joint_info(ospec.dataset).n_joints
# (spec, crops): the five BASELINE.json configs at full base width (+ stride 8 RN50, the non-centered variant)
CASES = [(ModelSpec(50, 32, 'h36m'), 2), (ModelSpec(50, 16, 'h36m'), 3), (ModelSpec(50, 16, 'many19'), 1),
         (ModelSpec(101, 8, 'many19'), 1), (ModelSpec(50, 4, 'h36m'), 1), (ModelSpec(50, 8, 'merged'), 1),
         (ModelSpec(50, 16, 'h36m', centered_stride=False), 1),
         # a second, harsher fp16 regime: conv3 at its undamped He initialisation (synth.RES_GAIN = 0.25 everywhere else keeps
         # the synthetic residual stream in the numeric range of a trained net); activations reach ~2e4 here
         (ModelSpec(50, 16, 'h36m'), 1, {'res_gain': 1.0}),
         # {'batch': N}: every launch at its REAL batch.  The call is built from the case's `crops` images, laid out by
         # H.crop_assignment: the oracle runs for them (positions 0 .. crops - 1; the last position of the call holds the last of
         # them) and EVERY position of every tensor must carry the bits of its twin.
         # The dispatch of calls with >= 128 crops (512-pixel 3x3 tiles, more layers on the 256 x 256 GEMM, from 256 crops the
         # 256-pixel head)
         (ModelSpec(50, 16, 'h36m'), 2, {'batch': 130}), (ModelSpec(50, 16, 'h36m'), 2, {'batch': 256}),
         # RAGGED calls: odd sizes that real calls have (boxes x views, N / world) and the batches above do not, each with a dispatch table
         # that holds none of 1, 8, 16, 32, 64, 128, 256 (dry run: tests/test_kernel_coverage.py, DryRun) -- on the oracle run of two crops
         # of the case in front of it where there is one ('pose_ratios': False as for C4 / C5 below).  Grids as the launchers compute
         # them (tiles of couts x tiles of pixels; conv_pws: one block per CU, `halves` blocks of 256 couts per tile stream).
         # 13 crops of RN50-s16 (the table of 13..15): 3328 pixels on 16 x 16 maps = 13 / 26 tiles.  Grids of 26 (block2/unit_4/conv2 on
         # 128 x 128 tiles), 52 (block3's conv2 and conv1 layers) and 260 blocks (the shortcut + conv1 pairs of block3 and block4): the
         # remainder arm of the XCD tile map with r = 2, 4, 4; conv_pws<k256> deals 104 tiles of 32 pixels to 64 tile streams
         (ModelSpec(50, 16, 'h36m'), 2, {'batch': 13, 'pose_ratios': False}),
         # 63 crops of RN50-s32 (a table of its own): 64-pixel images in block3 / block4, 4032 pixels = 31.5 tiles of 128 and 15.75 of
         # 256 -- the last tile of block3/unit_6's conv2 and conv3, of block4's pair, 3x3 and conv1 layers is ragged (64 of 128 and 192
         # of 256 pixels); conv_pws<k512> deals 126 tiles of 32 pixels to 32 tile streams; on 16 x 16 maps grids of 252 and 630 blocks
         # (r = 4, 6).  1.6 s and 2.0 s
         (ModelSpec(50, 32, 'h36m'), 2, {'batch': 63, 'pose_ratios': False}),
         # crop sides other than 256 (the model file's proc_side): 56/28/14/7-wide maps and a 7 x 7 head on the fp32-output GEMM +
         # two-launch soft-argmax (224); an 18 x 18 head of 424 channels (288); 96/48/24-wide maps (384); RN101-s8 on 80/40-wide
         # maps (320); block1 on 128-wide maps and a 16 x 16 head (512)
         (ModelSpec(50, 32, 'h36m', proc_side=224), 2),
         # ... and the same two crops in a call of 64: 49-pixel images, so every tile of block4 and of the f32out head GEMM crosses
         # image boundaries, and the two-launch soft-argmax at 64 crops (1.3 s; the batch-256 case above: 1.8 s, both on the oracle
         # run of the case in front of them; with its own oracle run the batch-130 case takes 2.8 s)
         (ModelSpec(50, 32, 'h36m', proc_side=224), 2, {'batch': 64}),
         (ModelSpec(50, 16, 'merged', proc_side=288), 1),
         (ModelSpec(50, 16, 'h36m', proc_side=384), 1), (ModelSpec(101, 8, 'many19', proc_side=320), 1),
         (ModelSpec(50, 32, 'h36m', proc_side=512), 1),
         # the 256-pixel head tiles on an 80 x 80 heat map (stride 4 at 320) at the real batch 16
         (ModelSpec(50, 4, 'h36m', proc_side=320), 2, {'batch': 16}),
         # the two configurations whose dilated 3x3 layers change tile shape (kc32: 512-pixel sub-grid tiles) exactly at their per-GPU
         # batch, C4 and C5 of BASELINE.json: every layer behind the first such one, with its own residual / shortcut / sub-sampling
         # flags, at that batch and on every crop (test_gpu_forward.py's batch-independence test stops comparing bits there).
         # 8.1 s and 15.3 s against the batch-256 case's 1.8 s (2.8 s with its oracle run), nearly all of it the CPU's fp16 model of two
         # crops on 32 x 32 / 64 x 64 maps (whole graph, then launch by launch); the GPU's share is under a second.  Cut for that:
         # 'pose_ratios': False -- no exact-math run, no pose ratios (9.0 s and 18.3 s with them); that criterion is applied to these
         # two configurations at these batches by test_batch_independence_of_the_other_baseline_configs.  No layer is left out: the
         # expensive ones (block3 / block4 behind the first kc32 layer) are what the cases are for.
         (ModelSpec(101, 8, 'many19'), 2, {'batch': 32, 'pose_ratios': False}),
         # ragged, as above: 13 crops of RN101-s8 (a table of its own: block3's 3x3 on 64-cout tiles with the 384-row slab, block4's
         # conv1 on conv_gemm4w quarter tiles behind a whole-tile pair) and 5 crops of RN50-s4 (a table of its own).  Their maps have 1024
         # and 4096 pixels from block2 / block1 on, so every tile grid is a multiple of 8 at ANY call size (>= 4 pixel tiles per image x
         # >= 2 cout tiles, 8 x 1 for 512-pixel tiles): no N reaches the remainder arm there.  What an odd call changes: the per-image
         # dimension of the head's grid (16 x 13, 64 x 5) and of the soft-argmax finalize (13 and 5 blocks), and tile counts that the
         # persistent kernels' streams do not divide (RN101-s8: 832 tiles of 64 pixels in conv_b1_chain, 416 of 32 in conv_pws<k256>).
         # 5.8 s and 12.1 s, the CPU's fp16 model of two crops as for the two cases they stand behind
         (ModelSpec(101, 8, 'many19'), 2, {'batch': 13, 'pose_ratios': False}),
         (ModelSpec(50, 4, 'h36m'), 2, {'batch': 16, 'pose_ratios': False}), (ModelSpec(50, 4, 'h36m'), 2, {'batch': 5, 'pose_ratios': False}),
         # the 128-pixel ring head with 144 weight rows (test_kernel_coverage.py: X-rn50-s8-J17-b32) behind its whole chain
         # (4.4 s; 5.1 s with the pose ratios)
         (ModelSpec(50, 8, 'h36m'), 2, {'batch': 32, 'pose_ratios': False})]
_id = lambda c: (f'rn{c[0].arch}-s{c[0].stride}-{c[0].dataset}-n{c[1]}' + ('' if c[0].proc_side == 256 else f'-side{c[0].proc_side}') +
                 ('' if c[0].centered_stride else '-nc') +
                 ('-undamped' if len(c) > 2 and 'res_gain' in c[2] else '') + (f'-of-batch{c[2]["batch"]}' if len(c) > 2 and 'batch' in c[2] else ''))


def case_params(spec, extra):
    """The bench / golden parameter set of `spec`, or (extra['res_gain']) the undamped variant with its logits kernel scaled
    to the same per-joint logit std (~4) by a one-crop run of the exact oracle."""
    if not extra or 'res_gain' not in extra:
        return synth.make_params(spec.arch, spec.n_head_channels, spec.base_width, seed=0,
                                 logit_gain=synth.logit_gain_for(spec.arch, spec.stride))
    mk = lambda lg: synth.make_params(spec.arch, spec.n_head_channels, spec.base_width, seed=0, logit_gain=lg, res_gain=extra['res_gain'])
    logits = OF.backbone_logits(H.oracle_spec(spec), mk(1.0), synth.make_images(1, spec.proc_side, seed=1234), torch.float64, None)
    return mk(round(4.0 / float(logits.std()), 6))


def ulp16(v):
    """Spacing of fp16 numbers at magnitude |v| (normal range; 2^-24 below it)."""
    v = np.maximum(np.abs(v), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(v)) - 10)


def layer_keys(name):
    """plan layer name -> (oracle key of the primary output, oracle key of the second output or None)."""
    if name == 'conv1+pool1':
        return 'pool1', None
    if name in ('conv1', 'pool1', 'logits'):
        return name, None
    if name.endswith('/conv1+conv2'):                    # conv1 runs on the 3x3 layer's LDS slab; layer dumps get a copy of its output
        return name[:-len('conv1+conv2')] + 'conv2', name[:-len('conv1+conv2')] + 'conv1'
    if name.endswith('/shortcut+conv1'):
        unit = name[:-len('/shortcut+conv1')]
        return unit + '/shortcut', unit + '/conv1'
    if '/conv3+' in name:
        unit, nxt = name.split('/conv3+')
        return unit, f'{unit.split("/")[0]}/{nxt}'
    if name.endswith('/conv3'):
        return name[:-len('/conv3')], None
    if name.endswith(('/conv1', '/conv2', '/shortcut')):
        return name, None
    return None, None


def compare_fp16(got, ref, what, chained=False, addend=None):
    """chained=False: got and ref were computed from the same inputs; chained=True: whole-graph comparison.
    addend: for a residual sum fp16(shortcut + fp16(conv)), the shortcut -- the flip happens at the magnitude of the
    conv term (<= |sum| + |shortcut|), which cancellation can leave far above the sum's own."""
    ref_max = float(np.abs(ref).max())
    err = np.abs(got - ref)
    worst = float(err.max()) / float(ulp16(ref_max))
    # elements far below the layer maximum (ReLU zeros, cancellations) carry the ABSOLUTE fp32-accumulation noise of
    # their dot product, not a relative one: their yardstick is floored at 1/64 of the maximum
    mag = np.maximum(np.maximum(np.abs(ref), np.abs(got)), ref_max / 64)
    if addend is not None:
        mag = 2.0 * np.maximum(mag, np.abs(addend))
    own = err / ulp16(mag)
    own_max = float(own.max())
    frac_equal = float((got == ref).mean())
    rep = os.environ.get('METRO_F16_REPORT')
    if rep:
        with open(rep, 'a') as f:
            f.write(f'{what}\t{int(chained)}\t{ref_max:.4g}\t{worst:.3f}\t{frac_equal:.5f}\t{own_max:.2f}\n')
        return worst, frac_equal
    if chained:
        assert worst <= CHAIN_ULPS_OF_MAX, f'{what}: {worst:.2f} ulps of the layer maximum {ref_max:.4g} (whole graph)'
    else:
        assert own_max <= 1.0, f'{what}: an element is {own_max:.2f} ulps of its own magnitude off (same inputs)'
        assert frac_equal >= MIN_IDENTICAL, f'{what}: only {frac_equal:.5f} of the elements bit-identical (same inputs)'
    return worst, frac_equal


def nhwc(t):
    return t.permute(0, 2, 3, 1).numpy()


_ORACLE = {}


def oracle_run(spec, params, n, res_gain, with_exact=True):
    """(images, collection, poses of the fp16 model, poses of exact math or None) of the first n synthetic crops: computed once
    per (spec, n, res_gain) and shared by the cases that differ in the batch only (the last one is kept; nothing writes to it)."""
    key = (spec, n, res_gain, with_exact)
    if not with_exact and (spec, n, res_gain, True) in _ORACLE:        # the run of the case in front, without its exact poses
        return _ORACLE[(spec, n, res_gain, True)][:3] + (None,)
    if key not in _ORACLE:
        _ORACLE.clear()
        images = synth.make_images(n, spec.proc_side, seed=4321)
        ospec = H.oracle_spec(spec)
        col = {}
        want = f16emu.forward(ospec, params, images, col).numpy()              # whole graph, fp16 model
        exact = OF.forward(ospec, params, images, torch.float64).numpy() if with_exact else None     # whole graph, exact
        _ORACLE[key] = (images, col, want, exact)
    return _ORACLE[key]


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_f16_mode_layerwise_against_fp16_oracle(cuda, case):
    spec, n = case[0], case[1]
    extra = case[2] if len(case) > 2 else {}
    params = case_params(spec, extra)
    batch = extra.get('batch', n)
    images, col, want, exact = oracle_run(spec, params, n, extra.get('res_gain'), extra.get('pose_ratios', True))
    # a real-batch case: position i of the call holds crop assign[i] of the n the oracle is computed for (positions 0 .. n - 1)
    assign = H.crop_assignment(batch, n, zlib.crc32(_id(case).encode()))
    all_images = H.lay_out_twins(images, assign)
    sel = list(range(n))
    ospec = H.oracle_spec(spec)
    root = f'MainPart/{ospec.arch_name}'
    units = {u.name: u for u in schedule(ospec)}
    order = list(units)
    x = torch.from_numpy(all_images).to(cuda)
    eng = Engine(spec, params, 'f16', max_batch=batch, device=cuda)
    hip = {}                                                               # oracle key -> the HIP path's tensor (NCHW fp64)

    def fetch(i, second=False):
        out = eng.forward_upto(x, i, second=second)
        H.assert_twins(out, assign, n, eng.layer_infos()[i].name.decode() + (' (second output)' if second else ''))
        return out[sel].cpu().double().permute(0, 3, 1, 2).contiguous()

    def unit_input(uname):
        k = order.index(uname)
        return hip['pool1'] if k == 0 else hip[order[k - 1]]

    checked = 0
    for i, li in enumerate(eng.layer_infos()):
        name = li.name.decode()
        if li.kind == _lib.LAYER_SOFTARGMAX:
            continue
        k1, k2 = layer_keys(name)
        assert k1 is not None and k1 in col, f'layer {name!r} has no oracle counterpart'
        got = fetch(i)
        hip[k1] = got
        if li.fused_flags & _lib.FUSED_CONV1_IN_FRONT:       # the 3x3's reference needs the launch's OWN conv1 output: dumped first
            hip[k2] = fetch(i, second=True)
        # ---- the oracle function of this tensor on the HIP path's own inputs -------------------------
        ref2 = addend = None
        if k1 == 'pool1':
            ref = f16emu.stem_pool(params, root, images)
        elif k1 == 'logits':
            ref = f16emu.head_logits(hip[order[-1]], params, root)
        else:
            uname = '/'.join(k1.split('/')[:2])
            unit, pre = units[uname], f'{root}/{uname}/bottleneck_v2'
            kind = k1[len(uname):]
            if kind == '/shortcut':
                ref = f16emu.unit_shortcut(unit_input(uname), params, pre, unit)
            elif kind == '/conv1':
                ref = f16emu.unit_conv1(unit_input(uname), params, pre)
            elif kind == '/conv2':
                ref = f16emu.unit_conv2(hip[uname + '/conv1'], params, pre, unit)
                if li.fused_flags & _lib.FUSED_CONV1_IN_FRONT:   # conv1 of the same launch, held to the model like any conv1
                    ref2 = f16emu.unit_conv1(unit_input(uname), params, pre)
            else:
                assert kind == '', k1
                # the shortcut is a tensor of the plan (projection), or computed by the oracle from the HIP path's own unit input:
                # identity shortcuts, and the projection computed inside the conv3 launch (METRO_FUSED_PROJECTION_SHORTCUT)
                sc = hip[uname + '/shortcut'] if uname + '/shortcut' in hip else \
                    f16emu.unit_shortcut(unit_input(uname), params, pre, unit)
                ref = f16emu.unit_conv3_add(hip[uname + '/conv2'], sc, params, pre)
                addend = nhwc(sc)
            if k2 is not None:
                u2 = '/'.join(k2.split('/')[:2])
                src = got if u2 != uname else unit_input(uname)             # next unit's conv1 reads THIS launch's output
                ref2 = f16emu.unit_conv1(src, params, f'{root}/{u2}/bottleneck_v2')
        assert tuple(got.shape) == tuple(ref.shape), (name, got.shape, ref.shape)
        if li.out_dtype == _lib.METRO_F16:
            compare_fp16(nhwc(got), nhwc(ref), name, addend=addend)
            compare_fp16(nhwc(got), nhwc(col[k1]), name, chained=True)
        else:                                                               # fp32 logits: fp32 accumulation noise only
            rel = float((got - ref).abs().max() / ref.abs().max())
            assert rel <= 2e-6, (name, rel)
            rel_chain = float((got - col[k1]).abs().max() / col[k1].abs().max())
            assert rel_chain <= 1e-2, (name, rel_chain)
        checked += 1
        if li.out2_offset >= 0:
            assert k2 is not None and k2 in col and ref2 is not None, f'second output of {name!r} has no oracle counterpart'
            got2 = fetch(i, second=True)
            hip[k2] = got2
            compare_fp16(nhwc(got2), nhwc(ref2), name + ' (second output)')
            compare_fp16(nhwc(got2), nhwc(col[k2]), name + ' (second output)', chained=True)
            checked += 1
    assert checked >= len(eng.layer_infos()) - 1
    # ---- soft-argmax on the HIP path's own logits, then the whole graph ---------------------------------
    poses = eng.forward(x)
    H.assert_twins(poses, assign, n, 'poses')
    poses = poses[sel].cpu().numpy()
    _, c01 = soft_argmax01(hip['logits'], ospec_joints(ospec), ospec.depth)
    d_sa = float(np.abs(poses - coords01_to_output(ospec, c01).numpy()).max())
    d_emu = float(np.abs(poses - want).max())
    if exact is None:        # a case without the exact-math run ('pose_ratios': False): every layer, the soft-argmax, no pose ratios
        print(f'\n[{_id(case)}] {checked} tensors; poses: |hip - softargmax64(hip logits)| {d_sa:.2e} mm, |hip - f16emu| {d_emu:.4f} mm')
        assert d_sa <= SOFTARGMAX_TOL_MM, d_sa
        return
    d_exact = float(np.abs(poses - exact).max())
    emu_exact = float(np.abs(want - exact).max())
    print(f'\n[{_id(case)}] {checked} tensors; poses: |hip - softargmax64(hip logits)| {d_sa:.2e} mm, |hip - f16emu| {d_emu:.4f} mm, '
          f'|hip - fp64| {d_exact:.3f} mm, |f16emu - fp64| {emu_exact:.3f} mm')
    rep = os.environ.get('METRO_F16_REPORT')
    if rep:
        with open(rep, 'a') as f:
            f.write(f'POSES {_id(case)}\t{d_sa:.3e}\t{d_emu:.4f}\t{d_exact:.3f}\t{emu_exact:.3f}\n')
        return
    assert d_sa <= SOFTARGMAX_TOL_MM, d_sa
    # two fp16 realisations of one graph are two samples of the same rounding noise (|hip - f16emu| is 0.3-2 mm here,
    # like either one's distance to exact math): the HIP path must be as ACCURATE as the fp16 model, not equal to it
    assert d_exact <= POSE_RATIO_MAX * emu_exact, (d_exact, emu_exact)
    assert np.abs(poses - exact).mean() <= POSE_RATIO * np.abs(want - exact).mean()
