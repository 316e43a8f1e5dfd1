"""The conv, head, pool and soft-argmax kernels on operands beyond 2^31 bytes, 2^32 bytes and 2^31 elements, against fp64.

The supported grid (tests/test_kernel_coverage.py: crop sides 64 .. 512, both archs, four strides, three heads, every call size
1 .. 256) reaches activations of 16 GiB in the f16 path (block4's output at stride 4, side 512, 256 crops) and of 64 GiB in the
f64 mode, while every other GPU case launches its large crop sides at small call sizes and its large call sizes at side 256 --
at most 2^32 bytes and 2^31 elements, one element short of where an `int` element index wraps.  The kernels hold pixel indices in
int and widen to size_t before the channel count goes in; per-lane 32-bit offsets (LDS-DMA, buffer loads) are taken against a
wave-uniform base of the tile.  These cases hold that on the device:

  * LARGE_CASES comes from the dry run of tests/test_kernel_coverage.py (large_operand_scan, large_address_cases): for every
    (kernel, operand role, class) triple the grid reaches -- class A beyond 2^31 bytes, B beyond 2^32 bytes, E beyond 2^31
    elements -- the (spec, call size, layer) with the fewest multiply-accumulates that puts LARGE_IMAGES_BEYOND = 4 whole images
    of that operand beyond the boundary.  test_large_operand_closure (CPU, next to test_pair_closure) holds the list to the grid.
    The parity modes' own range (tests/test_parity_coverage.py) reaches all three classes too (fp64 activations are four times
    the fp16 ones): their triples are in the list, launched through test_parity_coverage.parity_launch.
  * test_large_address_launch: one launch per case through the path of the single launches (test_kernel_coverage._launch:
    real layer shape at the real call size, NaN-filled outputs, the entry point must launch the id the plan names, every
    position carries its twin's bits, fp64 reference on the base images with the bars of that file: 2e-3 of the layer maximum
    for fp16 outputs, 2e-5 for fp32 ones, 2e-3 mm for poses; the parity cases with the exact set and the contract bound of
    their file).  What a case adds, and asserts itself: the images beyond each boundary, and a twin layout in which, for every
    triple the case is there for, some image beyond the boundary differs from the image one wrap distance below it
    (helpers.wrap_assignment) -- a load whose address wraps reads another image, a store that wraps leaves NaN above or
    overwrites another image below.  Base images: 4, or 2 where the fp64 reference of 4 would pass twice the heaviest reference
    of the existing single launches (large_base_images).  The twin check gathers and compares in groups of whole images
    (helpers.assert_twins): nothing of the test's own tooling indexes across 2^31 elements.
  * test_large_forward: RN50-s4-h36m at side 512 and 68 crops -- 4 images of block4's output beyond 2^32 bytes, a 15 GiB
    workspace -- through Engine.forward: the executor's slot offsets times n and the status words behind the last slot.

Measured on the MI355X: 25 launch cases + the forward take 29 s in all (15.6 s the 15 f16 cases, 12.8 s the 10 parity cases,
0.5 s the forward); the slowest f16 case 1.6 s, the slowest parity case 4.3 s (the first conv_igemm_f32 launch of the
process), against 0.9 s for the slowest existing single launch of test_kernel_coverage.py on the same run.  No case failed: the
address arithmetic holds as read.
"""
import time
import zlib

import numpy as np
import pytest
import torch

from metro_pose3d_amd import ModelSpec, synth
from metro_pose3d_amd.engine import Engine
from tests import helpers as H
from tests import test_kernel_coverage as KC
from tests.test_kernel_coverage import LARGE_CLASSES, LARGE_IMAGES_BEYOND, DryRun, spec_name

PRECISIONS = ('f16', 'f64', 'f32', 'f32m')

try:
    LARGE_CASES = KC._large_cases(PRECISIONS)
except Exception as e:  # noqa: BLE001  (library not built: tests/test_kernel_coverage.py reports it)
    LARGE_CASES = [pytest.param(None, None, 0, -1, str(e), {}, id='library-missing')]


def case_base_images(prec, li, n):
    """4 base images; 2 where the reference of 4 would cost too much (f16: KC.large_base_images; parity: that file's own rule)."""
    if prec == 'f16':
        return min(KC.large_base_images(li), n)
    from tests import test_parity_coverage as PC
    return min(PC.base_images(li) if li.kind == KC._lib.LAYER_CONV else 4, n)


def case_wraps(infos, i, kid, n, mine):
    """[(first image wholly beyond the boundary, wrap distance in images)] of the triples a case is there for, where the boundary
    is a whole number of images (else a wrapped access lands inside another image, at another pixel)."""
    roles = KC.operand_roles(infos, i, kid)
    out = set()
    for _, role, cls in mine:
        unit, bound = LARGE_CLASSES[cls]
        per = roles[role][0] * (roles[role][1] if unit == 'bytes' else 1)
        if bound % per == 0 and bound // per < n:
            out.add((bound // per, bound // per))
    return sorted(out)


TIMES = {}      # case id -> wall seconds (printed per case and summed by the last one)


@pytest.mark.gpu
@pytest.mark.parametrize('prec,spec,n,layer,kid,mine', LARGE_CASES)
def test_large_address_launch(lib, cuda, request, prec, spec, n, layer, kid, mine):
    assert spec is not None, f'libmetro_hip.so could not be loaded at collection time: {kid}'
    t0 = time.time()
    run = DryRun(spec, n, prec)
    li, name = run.infos[layer], run.names[layer]
    assert run.kernels(n, [layer]) == [kid]
    # what the case is there for: the operand is in the class at this call size, with the images beyond the boundary the list states
    now = KC.large_triples(run.infos, layer, kid, n)
    assert mine and all(now.get(t) == images for t, images in mine.items()), (mine, now)
    short = {t: images for t, images in mine.items() if images < LARGE_IMAGES_BEYOND}
    assert not short or n == KC.GRID_BATCHES[-1] or not any(t in KC.held_triples(c[3], c[6]) for t in short for c in KC.large_operand_scan(prec)), \
        f'fewer than {LARGE_IMAGES_BEYOND} images beyond the boundary below the largest call: {short}'
    p = case_base_images(prec, li, n)
    wraps = case_wraps(run.infos, layer, kid, n, mine)
    cname = f'{spec_name(spec)}-b{n}'
    assign, seed = H.wrap_assignment(n, p, zlib.crc32(f'{prec}/{cname}/{name}'.encode()), wraps)
    for first, d in wraps:
        assert any(assign[i] != assign[i - d] for i in range(first, n)), (first, d)
    try:
        if prec == 'f16':
            KC._launch(lib, cuda, cname, spec, n, layer, kid, assign=assign)
        else:
            from tests.test_parity_coverage import parity_launch
            parity_launch(lib, cuda, prec, spec, n, layer, kid, assign=assign)
    finally:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    TIMES[request.node.callspec.id] = dt = time.time() - t0
    beyond = ', '.join(f'{k} {role} {cls}: {images}' for (k, role, cls), images in sorted(mine.items()))
    print(f'\n[large address] {request.node.callspec.id}: call size {n}, {p} base images (seed {seed}), wraps (first image, distance) {wraps}; '
          f'images beyond each boundary -- {beyond}; wall {dt:.1f} s (sum so far {sum(TIMES.values()):.1f} s over {len(TIMES)} cases)')


FORWARD_SPEC = ModelSpec(50, 4, 'h36m', proc_side=512)
FORWARD_PARTS = 2       # the whole call against this many equal parts


def forward_call_size():
    """The smallest n that puts LARGE_IMAGES_BEYOND whole images of block4's output beyond 2^32 bytes."""
    run = DryRun(FORWARD_SPEC, 256)
    i = run.names.index('block4/unit_3/conv3')
    per = KC.operand_roles(run.infos, i, '')['output']
    return 2 ** 32 // (per[0] * per[1]) + LARGE_IMAGES_BEYOND, i


def test_large_forward_call_size():
    n, i = forward_call_size()
    assert n == 68
    run = DryRun(FORWARD_SPEC, n)
    assert KC.images_beyond(n, run.infos[i].out_bytes_per_image, 2 ** 32) == LARGE_IMAGES_BEYOND
    # the whole call and its parts run the same instantiations: the criterion between them is bit equality (test_large_forward)
    assert n % FORWARD_PARTS == 0 and run.kernels(n) == run.kernels(n // FORWARD_PARTS)
    assert 14 * 2 ** 30 < run.eng.workspace_bytes < 17 * 2 ** 30


@pytest.mark.gpu
def test_large_forward(cuda):
    """One whole forward whose workspace slots pass 4 GiB: every position's poses carry their twin's bits; the call equals its
    parts -- the criterion of tests/test_gpu_forward.py between a whole call and its parts where both run the same
    instantiations, torch.equal, which they do at 68 = 34 + 34 crops (asserted from the dry run, here and on the CPU); and
    metro_forward_status is clean, its words read from behind the last slot, above 4 GiB.  What holds the poses to exact math
    is the single launches above and the forward tests at side 256: the fp64 oracle of one 512-pixel crop at stride 4 is
    0.6 T multiply-accumulates."""
    t0 = time.time()
    spec = FORWARD_SPEC
    n, _ = forward_call_size()
    p = 4
    params = synth.make_params(spec.arch, spec.n_head_channels, spec.base_width, seed=0, logit_gain=synth.logit_gain_for(spec.arch, spec.stride))
    base = synth.make_images(p, spec.proc_side)
    first = n - LARGE_IMAGES_BEYOND                      # block4's output: the first image beyond 2^32 bytes; 2^31 bytes is half as far
    assign, seed = H.wrap_assignment(n, p, zlib.crc32(b'large forward'), [(first, first), (first // 2, first // 2)])
    x = H.lay_out_twins(torch.from_numpy(base).to(cuda), assign)
    eng = Engine(spec, params, 'f16', max_batch=n, device=cuda)
    m = n // FORWARD_PARTS
    try:
        assert eng.workspace_bytes > 14 * 2 ** 30 and int(eng.lib.metro_plan_status_offset(eng._plan)) > 2 ** 32
        assert eng.layer_kernels(n) == eng.layer_kernels(m)
        whole = eng.forward(x).clone()
        eng.check_finite(n)                              # metro_forward_status: raises when a word is set
        assert int(eng.status_words(n).sum()) == 0
        assert torch.isfinite(whole).all()
        H.assert_twins(whole, assign, p, 'poses of the whole call')
        assert (whole[:p] - whole[:p].mean(dim=0)).abs().max().item() > 1.0, 'the base images give one pose: the twin check holds nothing'
        parts = torch.cat([eng.forward(x[k * m:(k + 1) * m]).clone() for k in range(FORWARD_PARTS)])
        assert torch.equal(whole, parts), f'{n} crops in one call differ from {FORWARD_PARTS} x {m}: worst {(whole - parts).abs().max().item()} mm'
    finally:
        eng.close()
        del eng
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    print(f'\n[large address] whole forward {spec_name(spec)}: call size {n} (seed {seed}), {LARGE_IMAGES_BEYOND} images of block4\'s output beyond '
          f'2^32 bytes, twins bit-equal, whole == {FORWARD_PARTS} x {m} bit for bit, status clean; wall {time.time() - t0:.1f} s')
