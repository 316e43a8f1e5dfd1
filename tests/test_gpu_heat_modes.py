"""Per-joint heat-map modes on the MI355X: toy-width synthetic models (base_width 16) through Engine.forward_modes, held to
the fp64 restatement (tests/heat_modes_ref.py) of the logits of the SAME forward at the same n, read through the layer dump
(forward_upto) -- the comparisons are on identical values, so `voxel` is torch.equal -- on f16, f32m and f64 plans and at every
head shape at which the kernel takes another path: a volume of 32 voxels (S = 2), an odd side (S = 3, 7; 53 joints), volumes
staged whole (S = 16; 17 and 19 joints; depth 4), a volume staged in y-slabs with halo rows (S = 64: 13 rows a slab on fp32
logits, 5 on fp64), k = 1, 2 and 8, radius 0, 1 and 3, 1, 2 and 65 crops, more crops than one bound forward takes (heat_chunk).

Tolerances: profiles/heat_modes_parity.json records the worst deviation per precision and head (mass and peak in probability,
coords01 in grid steps, cov01 relative to one voxel's variance; tools/heat_modes_parity.py runs gpu_deviations() below); the
tests assert FOUR times those figures (heat_modes_ref.gate).  A mode whose mass in the restatement is below 1e-6 is compared in
voxel and mass only; every case asserts on the restatement that fewer than 5 % of its emitted modes are such."""
import ctypes as C

import numpy as np
import pytest
import torch

from metro_pose3d_amd import ModelSpec, _lib, synth
from metro_pose3d_amd._lib import check
from metro_pose3d_amd.engine import Engine
from tests import helpers as H, heat_modes_ref as MR
from tests.test_gpu_heat_marginals import HEAT_IDS

pytestmark = pytest.mark.gpu

PRECISIONS = ('f16', 'f32m', 'f64')
# id -> (stride, proc_side, dataset, depth, the crops per call, k, radius)
HEADS = {
    'S2': (32, 64, 'h36m', 8, (1, 2, 65), 8, 3),
    'S3': (32, 96, 'h36m', 8, (2, 65), 2, 0),
    'S7-j53': (32, 224, 'merged', 8, (2,), 8, 1),
    'S16-j17': (16, 256, 'h36m', 8, (1, 2), 2, 1),
    'S16-j19': (16, 256, 'many19', 8, (2,), 8, 0),
    'S64': (4, 256, 'h36m', 8, (1,), 8, 3),
    'S8-d4': (16, 128, 'h36m', 4, (2,), 1, 3),
}
MODES_IDS = {'f16': 'heat_modes<acc32,logits32>', 'f32': 'heat_modes<acc64,logits32>', 'f32m': 'heat_modes<acc64,logits32>',
             'f64': 'heat_modes<acc64,logits64>'}
PLAIN = ('out', 'coords01', 'cov01', 'peak')


def make_case(head, seed=1):
    stride, side, dataset, depth, ns, k, radius = HEADS[head]
    spec = ModelSpec(50, stride, dataset, depth=depth, proc_side=side, base_width=16)
    params = synth.make_params(50, spec.n_head_channels, 16, seed=seed, logit_gain=synth.logit_gain_for(50, stride, 16))
    return spec, params, ns, k, radius


def buffers(eng, n, cuda, heat=False):
    sk = eng.spec.skeleton
    f32 = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=cuda)
    b = dict(out=f32(n, sk.n_out, 3), coords01=f32(n, sk.n_head, 3), cov01=f32(n, sk.n_head, 6), peak=f32(n, sk.n_head))
    if heat:
        xy_shape, z_shape = eng.heat_shapes(n)
        b.update(heat_xy=f32(*xy_shape), heat_z=f32(*z_shape))
    return b


def same(a, b):
    """Bit equality of two float tensors (NaN rows of missing modes included)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run_bound(eng, x, k, radius, cuda):
    """-> (the bound call's tensors with 'voxel' and 'stats', the unbound call's, the restatement of the same forward's dumped
    logits).  With eng.heat_chunk set the bound call is made of forwards of at most that many crops: the unbound call and the
    dump are made of the same."""
    n, spec = x.shape[0], eng.spec
    b = buffers(eng, n, cuda)
    _, b['voxel'], b['stats'] = eng.forward_modes(x, k, radius, **b)
    u = buffers(eng, n, cuda)
    step = eng.heat_chunk or n
    dumps = []
    for i in range(0, n, step):
        eng.forward(x[i:i + step], **{key: u[key][i:i + step] for key in PLAIN})
        dumps.append(eng.forward_upto(x[i:i + step], len(eng.layer_infos()) - 2).cpu().numpy())
    ref = MR.modes(np.concatenate(dumps), spec.skeleton.n_head, spec.depth, list(spec.skeleton.permutation), k, radius)
    return b, u, ref


def hold(b, u, ref, spec, key, what):
    small = MR.small_fraction(*ref)
    print(f'heat_modes {key} {what}: {int((ref[0] >= 0).sum())} modes emitted, {small:.3f} of them below {MR.SMALL_MASS:g}')
    assert (ref[0][..., 0] >= 0).all() and small < 0.05, (what, small)
    MR.check(b['voxel'].cpu().numpy(), b['stats'].cpu().numpy(), ref[0], ref[1], spec.heatmap_side, spec.depth, key, what)
    for k in PLAIN:
        assert torch.equal(b[k], u[k]), (what, k)


def gpu_deviations(cuda):
    """{key: {'prob', 'grid', 'cov'}} of every comparison of this file: what tools/heat_modes_parity.py records."""
    out = {}
    for precision in PRECISIONS:
        for head in HEADS:
            spec, params, ns, k, radius = make_case(head)
            eng = Engine(spec, params, precision, max_batch=max(ns), device=cuda)
            worst = {'prob': 0.0, 'grid': 0.0, 'cov': 0.0}
            inputs = [torch.from_numpy(synth.make_images(n, spec.proc_side, seed=7)).to(cuda) for n in ns]
            if head == UINT8_HEAD and precision in UINT8_PRECISIONS:
                inputs.append(uint8_crops(spec, cuda))
            for x in inputs:
                for chunk in ((None, 32) if x.shape[0] > 32 else (None,)):
                    eng.heat_chunk = chunk
                    b, _, ref = run_bound(eng, x, k, radius, cuda)
                    assert np.array_equal(b['voxel'].cpu().numpy(), ref[0]), (precision, head, 'voxel')
                    dev = MR.deviation(b['stats'].cpu().numpy(), ref[0], ref[1], spec.heatmap_side, spec.depth)
                    worst = {m: max(worst[m], dev[m]) for m in worst}
                    print(f'gpu/{precision}/{head} n{x.shape[0]} chunk {chunk}: small-mass share {MR.small_fraction(*ref):.3f}', flush=True)
            eng.close()
            out[f'gpu/{precision}/{head}'] = worst
    return out


UINT8_HEAD, UINT8_PRECISIONS = 'S16-j17', ('f16', 'f32m')


def uint8_crops(spec, cuda):
    return torch.from_numpy(np.round(synth.make_images(2, spec.proc_side, seed=8) * 255).astype(np.uint8)).to(cuda)


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('head', list(HEADS))
def test_bound_forward_against_the_logits_of_the_same_forward(cuda, lib, head, precision):
    spec, params, ns, k, radius = make_case(head)
    eng = Engine(spec, params, precision, max_batch=max(ns), device=cuda)
    key = f'gpu/{precision}/{head}'
    for n in ns:
        x = torch.from_numpy(synth.make_images(n, spec.proc_side, seed=7)).to(cuda)
        for chunk in ((None, 32) if n > 32 else (None,)):          # 65 crops: one bound forward, and 32 + 32 + 1
            eng.heat_chunk = chunk
            b, u, ref = run_bound(eng, x, k, radius, cuda)
            hold(b, u, ref, spec, key, f'n{n} chunk {chunk}')
            if chunk is not None:                                   # the status words are the call's, not the last chunk's
                assert eng.status_words(n).shape == (n,) and not eng.status_words(n).any()
    eng.heat_chunk = None
    # modes and heat-maps bound together: each output has the bits it has when bound alone
    n = ns[-1]
    x = torch.from_numpy(synth.make_images(n, spec.proc_side, seed=7)).to(cuda)
    alone = buffers(eng, n, cuda)
    _, alone['voxel'], alone['stats'] = eng.forward_modes(x, k, radius, **alone)
    heat = buffers(eng, n, cuda, heat=True)
    eng.forward(x, **heat)
    # what the forward enqueues: unbound, the plan's own list; bound, the heat launches behind it
    plan_ids = ' & '.join(eng.layer_kernels(n))
    check(lib.metro_kernel_notes(1), 'notes')
    eng.forward(x)
    unbound_ids = lib.metro_last_kernel_id().decode()
    check(lib.metro_kernel_notes(1), 'notes')
    eng.forward_modes(x, k, radius)
    bound_ids = lib.metro_last_kernel_id().decode()
    check(lib.metro_kernel_notes(1), 'notes')
    both = buffers(eng, n, cuda, heat=True)
    _, both['voxel'], both['stats'] = eng.forward_modes(x, k, radius, **both)
    both_ids = lib.metro_last_kernel_id().decode()
    check(lib.metro_kernel_notes(0), 'notes')
    assert unbound_ids == plan_ids, (unbound_ids, plan_ids)
    assert bound_ids == plan_ids + ' & ' + MODES_IDS[precision], bound_ids
    # (that call also asked for cov01 and peak: its head and finalize launches are the MOMENTS instantiations)
    assert both_ids.endswith(' & ' + HEAT_IDS[precision] + ' & ' + MODES_IDS[precision]), both_ids[-200:]
    assert both_ids.count(' & ') == plan_ids.count(' & ') + 4, both_ids
    assert torch.equal(both['voxel'], alone['voxel']) and same(both['stats'], alone['stats'])
    for key in PLAIN + ('heat_xy', 'heat_z'):
        assert torch.equal(both[key], heat[key]), key
    eng.close()


@pytest.mark.parametrize('precision', UINT8_PRECISIONS)
def test_uint8_crops(cuda, precision):
    """f16 reads the bytes in its first kernel (metro_forward_u8), the parity precisions expand them first: both bound."""
    spec, params, _, k, radius = make_case(UINT8_HEAD)
    eng = Engine(spec, params, precision, max_batch=2, device=cuda)
    b, u, ref = run_bound(eng, uint8_crops(spec, cuda), k, radius, cuda)
    hold(b, u, ref, spec, f'gpu/{precision}/{UINT8_HEAD}', 'uint8')
    eng.close()


def raw_outputs(eng, n, k, cuda):
    nj = eng.spec.skeleton.n_out
    return (torch.full((n, nj, k), -7, dtype=torch.int32, device=cuda),
            torch.full((n, nj, k, MR.STATS), -7.0, dtype=torch.float32, device=cuda))


def test_rebinding_and_unbinding_between_enqueues(cuda, lib):
    """Binding is host state read at enqueue: A bound, forward 1, B bound (another k and radius), forward 2, unbound, forward 3,
    one synchronisation -- A holds the modes of forward 1, B those of forward 2, and forward 3 wrote neither."""
    spec, params, _, k, radius = make_case('S16-j17')
    eng = Engine(spec, params, 'f16', max_batch=2, device=cuda)
    x1 = torch.from_numpy(synth.make_images(2, spec.proc_side, seed=9)).to(cuda)
    x2 = torch.from_numpy(synth.make_images(1, spec.proc_side, seed=10)).to(cuda)
    want_pose, want1_v, want1_s = eng.forward_modes(x1, k, radius)
    _, want2_v, want2_s = eng.forward_modes(x2, 3, 0)
    (av, as_), (bv, bs) = raw_outputs(eng, 2, k, cuda), raw_outputs(eng, 2, 3, cuda)
    scratch = torch.empty(lib.metro_plan_modes_scratch_bytes(eng._plan, 2), dtype=torch.uint8, device=cuda)
    poses = torch.empty((2, spec.skeleton.n_out, 3), device=cuda)
    stream = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    fwd = lambda x: check(lib.metro_forward(eng._plan, H.ptr(x), x.shape[0], H.ptr(poses), H.ptr(eng._ws), stream), 'metro_forward')
    torch.cuda.synchronize()
    check(lib.metro_plan_bind_modes(eng._plan, H.ptr(av), H.ptr(as_), H.ptr(scratch), 2, k, radius), 'bind')
    fwd(x1)
    check(lib.metro_plan_bind_modes(eng._plan, H.ptr(bv), H.ptr(bs), H.ptr(scratch), 2, 3, 0), 'bind')
    fwd(x2)
    check(lib.metro_plan_bind_modes(eng._plan, None, None, None, 0, 0, 0), 'unbind')
    fwd(x1)
    torch.cuda.synchronize()
    assert torch.equal(av, want1_v) and same(as_, want1_s)
    assert torch.equal(bv[:1], want2_v) and same(bs[:1], want2_s)
    assert (bv[1:] == -7).all() and (bs[1:] == -7).all()                  # rows n .. max_n - 1 are not touched
    assert torch.equal(poses, want_pose)
    eng.close()


def test_more_crops_than_bound_are_refused_before_any_launch(cuda, lib):
    spec, params, _, k, radius = make_case('S16-j17')
    eng = Engine(spec, params, 'f16', max_batch=2, device=cuda)
    x = torch.from_numpy(synth.make_images(2, spec.proc_side, seed=9)).to(cuda)
    vx, st = raw_outputs(eng, 1, k, cuda)
    scratch = torch.empty(lib.metro_plan_modes_scratch_bytes(eng._plan, 1), dtype=torch.uint8, device=cuda)
    poses = torch.full((2, spec.skeleton.n_out, 3), -7.0, device=cuda)
    stream = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    check(lib.metro_plan_bind_modes(eng._plan, H.ptr(vx), H.ptr(st), H.ptr(scratch), 1, k, radius), 'bind')
    try:
        check(lib.metro_kernel_notes(1), 'notes')
        assert lib.metro_forward(eng._plan, H.ptr(x), 2, H.ptr(poses), H.ptr(eng._ws), stream) == -1
        assert b'bound mode buffers' in lib.metro_last_error() and lib.metro_last_kernel_id() == b''
    finally:
        check(lib.metro_kernel_notes(0), 'notes')
        check(lib.metro_plan_bind_modes(eng._plan, None, None, None, 0, 0, 0), 'unbind')
    torch.cuda.synchronize()
    assert (poses == -7).all() and (vx == -7).all() and (st == -7).all()
    eng.close()


def test_metro_forward_with_modes_bound_keeps_to_a_side_stream(cuda, lib):
    """The protocol of tests/stream_harness.py on metro_forward with modes bound (a chain: the bound buffers are no arguments of the
    entry): on a non-blocking side stream, behind the delay, the call returns while the delay runs and poses, voxel and stats have
    the bits of the default-stream run."""
    from tests import stream_harness as SH
    spec, params, _, k, radius = make_case('S16-j17')
    eng = Engine(spec, params, 'f16', max_batch=2, device=cuda)
    scratch = torch.empty(lib.metro_plan_modes_scratch_bytes(eng._plan, 2), dtype=torch.uint8, device=cuda)

    def fn(images):
        vx, st = raw_outputs(eng, 2, k, cuda)
        poses = torch.empty((2, spec.skeleton.n_out, 3), device=cuda)
        check(lib.metro_plan_bind_modes(eng._plan, H.ptr(vx), H.ptr(st), H.ptr(scratch), 2, k, radius), 'bind')
        try:
            check(lib.metro_forward(eng._plan, H.ptr(images), 2, H.ptr(poses), H.ptr(eng._ws),
                                    C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)), 'metro_forward')
        finally:
            check(lib.metro_plan_bind_modes(eng._plan, None, None, None, 0, 0, 0), 'unbind')
        return poses, vx, st
    a, b = (torch.from_numpy(synth.make_images(2, spec.proc_side, seed=s)).to(cuda) for s in (11, 12))
    SH.verdict(SH.Chain(fn, [a], [b]), cuda, what='metro_forward, modes bound', asynchronous=True, busy=False).require_ok()
    eng.close()


def test_nonfinite_logits_poison_their_joint_only(cuda):
    """A NaN bias on one logits channel: all modes of its joint are voxel -1 with NaN floats in every crop, every other joint
    keeps the bits of the clean model, and poses, statistics and status words are the unbound call's."""
    spec, params, _, k, radius = make_case('S16-j17')
    nj, bad_joint = spec.skeleton.n_head, 2
    x = torch.from_numpy(synth.make_images(2, spec.proc_side, seed=12)).to(cuda)
    eng = Engine(spec, params, 'f16', max_batch=2, device=cuda)
    _, clean_v, clean_s = eng.forward_modes(x, k, radius)
    torch.cuda.synchronize()
    eng.close()
    poisoned = dict(params)
    bias = params['MainPart/resnet_v2_50/logits/biases'].copy()
    bias[1 * nj + bad_joint] = np.nan
    poisoned['MainPart/resnet_v2_50/logits/biases'] = bias
    eng = Engine(spec, poisoned, 'f16', max_batch=2, device=cuda)
    b, u = buffers(eng, 2, cuda), buffers(eng, 2, cuda)
    _, vx, st = eng.forward_modes(x, k, radius, **b)
    words = eng.status_words(2).clone()
    eng.forward(x, **u)
    assert words.tolist() == [1, 1] and torch.equal(eng.status_words(2), words)
    rows = torch.tensor([p == bad_joint for p in spec.skeleton.permutation], device=cuda)
    assert rows.any() and not rows.all()
    assert (vx[:, rows] == -1).all() and torch.isnan(st[:, rows]).all()
    assert torch.equal(vx[:, ~rows], clean_v[:, ~rows]) and same(st[:, ~rows], clean_s[:, ~rows])
    for key in PLAIN:
        assert torch.equal(b[key].nan_to_num(nan=-7.0), u[key].nan_to_num(nan=-7.0)), key
    eng.close()


def test_forward_modes_in_chunks_equals_the_chunks_done_by_hand(cuda):
    spec, params, _, k, radius = make_case('S16-j17')
    eng = Engine(spec, params, 'f16', max_batch=3, device=cuda)
    x = torch.from_numpy(synth.make_images(3, spec.proc_side, seed=14)).to(cuda)
    by_hand = [eng.forward_modes(x[i:i + 1], k, radius) for i in range(3)]
    eng.heat_chunk = 1
    poses, vx, st = eng.forward_modes(x, k, radius)
    eng.heat_chunk = None
    for i, want in enumerate(zip(*by_hand)):
        assert same((poses, vx, st)[i], torch.cat(want)), i
    assert eng.status_words(3).shape == (3,) and not eng.status_words(3).any()
    eng.close()


def test_estimate_pose_modes_is_forward_modes_and_the_metric_conversion(cuda, tmp_path):
    from metro_pose3d_amd import inference as INF, save_model
    spec, params, _, _, _ = make_case('S16-j17')
    path = str(tmp_path / 'm.npz')
    save_model(path, spec, params)
    x = torch.from_numpy(synth.make_images(3, spec.proc_side, seed=13)).to(cuda)
    plain = INF.estimate_pose(x, path, return_uncertainty=True, return_heatmaps=True)
    res = INF.estimate_pose_modes(x, path, 3, 1, return_uncertainty=True, return_heatmaps=True)
    short = INF.estimate_pose_modes(x, path)
    assert len(res) == 6 and len(short) == 4 and isinstance(res[-1], INF.Modes) and isinstance(short[-1], INF.Modes)
    assert torch.equal(res[0], plain[0]) and torch.equal(short[0], plain[0])
    assert np.array_equal(res[1], plain[1]) and list(res[2]) == list(plain[2])
    assert torch.equal(res[3].covariance, plain[3].covariance) and torch.equal(res[3].peak, plain[3].peak)
    assert torch.equal(res[4].xy, plain[4].xy) and torch.equal(res[4].z, plain[4].z)
    assert short[-1].poses.shape == (3, spec.skeleton.n_out, 2, 3)
    # the composition, written out in torch: heatmap_to_metric of the mode, minus that of the root joint's mean
    eng = Engine(spec, params, 'f16', max_batch=8, device=cuda)
    c01 = torch.empty((3, spec.skeleton.n_head, 3), device=cuda)
    _, vx, st = eng.forward_modes(x, 3, 1, coords01=c01)
    last = spec.proc_side - 1
    lrc, half, box, side = last - last % spec.stride - 1, spec.stride // 2, spec.box_size_mm, spec.proc_side
    mm = lambda c: torch.cat([(c[..., :2] * lrc + half) * box / side, c[..., 2:] * box], -1)
    want = (mm(st[..., 2:5].double()) - mm(c01.double()[:, -1])[:, None, None]).float()
    m = res[-1]
    assert torch.equal(m.voxel, vx) and same(m.mass, st[..., 0]) and same(m.peak, st[..., 1]) and same(m.poses, want)
    s = torch.tensor([lrc * box / side, lrc * box / side, box], dtype=torch.float64, device=cuda)
    idx = torch.tensor([[5, 8, 9], [8, 6, 10], [9, 10, 7]], device=cuda)
    cov = (st.double()[..., idx] * (s[:, None] * s[None, :])).float()
    assert same(m.covariance, cov)
    on = vx >= 0
    assert on[..., 0].all() and (m.mass[on] > 0).all() and (m.mass.sum(-1) <= 1 + 1e-5).all()
    # a joint whose modes hold (nearly) all its mass: the plain pose is their mass-weighted blend
    full = m.mass.sum(-1) > 0.999
    if full.any():
        blend = (m.mass[..., None].double() * m.poses.double()).nan_to_num().sum(2)
        # what is missing: at most 0.001 of the mass, anywhere in the box, of the joint and of the root's share of the blend
        assert (blend - res[0].double())[full].abs().max() < 0.002 * box
    img = str(tmp_path / 'img.npy')
    np.save(img, x[0].cpu().numpy())
    INF.main(['--model-path', path, '--image', img, '--modes', '3,1'])
    eng.close()
    INF.clear_cache()
