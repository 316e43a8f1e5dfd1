"""Per-joint heat-map marginals on the MI355X: toy-width synthetic models (base_width 16) through Engine.forward with the
outputs bound, held to the fp64 restatement (tests/heat_marginals_ref.py) of the logits of the SAME forward at the same n, read
through the layer dump (forward_upto) -- which isolates the three new kernels from the network in front of them -- in all four
precisions and at every head shape at which the kernels take another path: a map smaller than a tile (S = 2, 3), a ragged
second tile (S = 7, with the 53-joint head whose rows are staged in several chunks), whole tiles (S = 16; J = 17 and 19),
64-pixel tiles (S = 64), depth 4, several crops, more crops than one bound forward takes (heat_chunk).

Tolerances.  Marginals: profiles/heat_marginals_parity.json records the worst deviation per precision and head (absolute, in
probability, and relative to the row's largest entry; tools/heat_marginals_parity.py runs gpu_deviations() below); the tests
assert FOUR times that figure, which heat_marginals_ref.gate holds below the probability of one voxel of a flat map.
Row sums and expectations compare two fp32 summations (f16 plans) of at most S*S*D non-negative terms each, done in chains of
at most ~136 terms (a tile's 64 pixels, 64 tiles, D depths, the slabs of the soft-argmax): 136 * 2^-24 = 8e-6 per sum,
numerator and normaliser on both sides -> 3.2e-5; asserted at 1e-4.  fp64 accumulators leave the fp32 roundings of the
outputs: S*S values of relative error 2^-24 each sum to at most 6e-8 of a total <= 1, twice -> asserted at 1e-6."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from metro_pose3d_amd import ModelSpec, _lib, synth
from metro_pose3d_amd._lib import check
from metro_pose3d_amd.engine import Engine
from tests import helpers as H, heat_marginals_ref as HR

pytestmark = pytest.mark.gpu

PRECISIONS = ('f16', 'f32', 'f32m', 'f64')
# id -> (stride, proc_side, dataset, depth, the crops per call)
HEADS = {
    'S2': (32, 64, 'h36m', 8, (1, 2, 65)),
    'S3': (32, 96, 'h36m', 8, (2, 65)),
    'S7-j53': (32, 224, 'merged', 8, (2,)),
    'S16-j17': (16, 256, 'h36m', 8, (1, 2)),
    'S16-j19': (16, 256, 'many19', 8, (2,)),
    'S64': (4, 256, 'h36m', 8, (1,)),
    'S8-d4': (16, 128, 'h36m', 4, (2,)),
}
SUM_TOL = {'f16': 1e-4, 'f32': 1e-6, 'f32m': 1e-6, 'f64': 1e-6}
HEAT_IDS = {'f16': 'heat_partial<acc32,logits32> & heat_fold<acc32> & heat_xy<acc32,logits32>',
            'f32': 'heat_partial<acc64,logits32> & heat_fold<acc64> & heat_xy<acc64,logits32>',
            'f32m': 'heat_partial<acc64,logits32> & heat_fold<acc64> & heat_xy<acc64,logits32>',
            'f64': 'heat_partial<acc64,logits64> & heat_fold<acc64> & heat_xy<acc64,logits64>'}


def make_case(head, seed=1):
    stride, side, dataset, depth, ns = HEADS[head]
    spec = ModelSpec(50, stride, dataset, depth=depth, proc_side=side, base_width=16)
    params = synth.make_params(50, spec.n_head_channels, 16, seed=seed, logit_gain=synth.logit_gain_for(50, stride, 16))
    return spec, params, ns


def buffers(eng, n, cuda):
    sk = eng.spec.skeleton
    f32 = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=cuda)
    xy_shape, z_shape = eng.heat_shapes(n)
    return dict(out=f32(n, sk.n_out, 3), coords01=f32(n, sk.n_head, 3), cov01=f32(n, sk.n_head, 6), peak=f32(n, sk.n_head),
                heat_xy=f32(*xy_shape), heat_z=f32(*z_shape))


def run_bound(eng, x, cuda):
    """-> (the bound call's tensors, the unbound call's, the restatement of the same forward's dumped logits).  With
    eng.heat_chunk set the bound call is made of forwards of at most that many crops (the kernels a forward dispatches follow
    its batch, so those are other forwards than one of all n crops): the unbound call and the dump are made of the same."""
    n, spec = x.shape[0], eng.spec
    b = buffers(eng, n, cuda)
    eng.forward(x, **b)
    u = buffers(eng, n, cuda)
    step = eng.heat_chunk or n
    dumps = []
    for i in range(0, n, step):
        eng.forward(x[i:i + step], **{k: u[k][i:i + step] for k in ('out', 'coords01', 'cov01', 'peak')})
        dumps.append(eng.forward_upto(x[i:i + step], len(eng.layer_infos()) - 2).cpu().numpy())
    logits = np.concatenate(dumps)
    ref = HR.marginals(logits, spec.skeleton.n_head, spec.depth, list(spec.skeleton.permutation))
    return b, u, ref


def hold(b, u, ref, spec, precision, key, what):
    xy, z = b['heat_xy'].cpu().numpy(), b['heat_z'].cpu().numpy()
    assert np.isfinite(xy).all() and np.isfinite(z).all(), what
    HR.check(xy, z, ref[0], ref[1], key, spec.heatmap_side ** 2 * spec.depth, what)
    tol = SUM_TOL[precision]
    sums = np.abs(xy.astype(np.float64).sum((2, 3)) - 1).max(), np.abs(z.astype(np.float64).sum(2) - 1).max()
    perm = list(spec.skeleton.permutation)
    mean = np.abs(HR.expectations(xy, z) - b['coords01'].cpu().numpy().astype(np.float64)[:, perm]).max()
    print(f'heat_marginals {key} {what}: row sums off by {sums[0]:.2e} / {sums[1]:.2e}, expectations by {mean:.2e} (bound {tol:.0e})')
    assert max(sums) <= tol and mean <= tol, (what, sums, mean)
    for k in ('out', 'coords01', 'cov01', 'peak'):
        assert torch.equal(b[k], u[k]), (what, k)


def gpu_deviations(cuda):
    """{key: (abs, rel, S*S*D)} of every marginal comparison of this file: what tools/heat_marginals_parity.py records."""
    out = {}
    for precision in PRECISIONS:
        for head in HEADS:
            spec, params, ns = make_case(head)
            eng = Engine(spec, params, precision, max_batch=max(ns), device=cuda)
            worst = [0.0, 0.0]
            inputs = [torch.from_numpy(synth.make_images(n, spec.proc_side, seed=7)).to(cuda) for n in ns]
            if head == UINT8_HEAD and precision in UINT8_PRECISIONS:
                inputs.append(uint8_crops(spec, cuda))
            for x in inputs:
                for chunk in ((None, 32) if x.shape[0] > 32 else (None,)):
                    eng.heat_chunk = chunk
                    b, _, ref = run_bound(eng, x, cuda)
                    for got, r in ((b['heat_xy'], ref[0]), (b['heat_z'], ref[1])):
                        a, rel = HR.deviation(got.cpu().numpy(), r)
                        worst = [max(worst[0], a), max(worst[1], rel)]
            eng.close()
            out[f'gpu/{precision}/{head}'] = (worst[0], worst[1], spec.heatmap_side ** 2 * spec.depth)
    spec, params, images, oracle_logits = golden_case()
    eng = Engine(spec, params, 'f64', max_batch=len(images), device=cuda)
    b = buffers(eng, len(images), cuda)
    eng.forward(torch.from_numpy(images).to(cuda), **b)
    ref = HR.marginals(oracle_logits, spec.skeleton.n_head, spec.depth, list(spec.skeleton.permutation))
    a = [HR.deviation(b[k].cpu().numpy(), r) for k, r in (('heat_xy', ref[0]), ('heat_z', ref[1]))]
    eng.close()
    out['gpu/f64/golden-oracle'] = (max(a[0][0], a[1][0]), max(a[0][1], a[1][1]), spec.heatmap_side ** 2 * spec.depth)
    return out


GOLDEN = 'toy-rn50-s16-w16-noncentered'
UINT8_HEAD, UINT8_PRECISIONS = 'S16-j17', ('f16', 'f32m')


def uint8_crops(spec, cuda):
    return torch.from_numpy(np.round(synth.make_images(2, spec.proc_side, seed=8) * 255).astype(np.uint8)).to(cuda)


def golden_case():
    """The committed golden toy case and the fp64 oracle's logits of it, NHWC."""
    from oracle import forward as OF
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'golden_poses_v1.npz'))
    m = json.loads(bytes(z['__meta__']).decode())[GOLDEN]
    spec = ModelSpec(**m['spec'])
    params = synth.make_params(spec.arch, spec.n_head_channels, spec.base_width, seed=m['param_seed'], logit_gain=m['logit_gain'])
    images = synth.make_images(m['batch'], spec.proc_side, seed=m['image_seed'])
    logits = OF.backbone_logits(H.oracle_spec(spec), params, images, torch.float64).permute(0, 2, 3, 1).contiguous().numpy()
    return spec, params, images, logits


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('head', list(HEADS))
def test_bound_forward_against_the_logits_of_the_same_forward(cuda, lib, head, precision):
    spec, params, ns = make_case(head)
    eng = Engine(spec, params, precision, max_batch=max(ns), device=cuda)
    key = f'gpu/{precision}/{head}'
    for n in ns:
        x = torch.from_numpy(synth.make_images(n, spec.proc_side, seed=7)).to(cuda)
        for chunk in ((None, 32) if n > 32 else (None,)):          # 65 crops: one bound forward, and 32 + 32 + 1
            eng.heat_chunk = chunk
            b, u, ref = run_bound(eng, x, cuda)
            hold(b, u, ref, spec, precision, key, f'n{n} chunk {chunk}')
            if chunk is not None:                                   # the status words are the call's, not the last chunk's
                assert eng.status_words(n).shape == (n,) and not eng.status_words(n).any()
    eng.heat_chunk = None
    # what the forward enqueues: unbound, the plan's own list; bound, the three heat launches behind it
    n = ns[-1]
    x = torch.from_numpy(synth.make_images(n, spec.proc_side, seed=7)).to(cuda)
    plan_ids = ' & '.join(eng.layer_kernels(n))
    check(lib.metro_kernel_notes(1), 'notes')
    eng.forward(x)
    unbound_ids = lib.metro_last_kernel_id().decode()
    check(lib.metro_kernel_notes(1), 'notes')
    b = buffers(eng, n, cuda)
    eng.forward(x, heat_xy=b['heat_xy'], heat_z=b['heat_z'])
    bound_ids = lib.metro_last_kernel_id().decode()
    check(lib.metro_kernel_notes(0), 'notes')
    assert unbound_ids == plan_ids, (unbound_ids, plan_ids)
    assert bound_ids == plan_ids + ' & ' + HEAT_IDS[precision], bound_ids
    eng.close()


@pytest.mark.parametrize('precision', UINT8_PRECISIONS)
def test_uint8_crops(cuda, precision):
    """f16 reads the bytes in its first kernel (metro_forward_u8), the parity precisions expand them first: both bound."""
    spec, params, _ = make_case(UINT8_HEAD)
    eng = Engine(spec, params, precision, max_batch=2, device=cuda)
    b, u, ref = run_bound(eng, uint8_crops(spec, cuda), cuda)
    hold(b, u, ref, spec, precision, f'gpu/{precision}/{UINT8_HEAD}', 'uint8')
    eng.close()


def test_rebinding_and_unbinding_between_enqueues(cuda, lib):
    """Binding is host state read at enqueue: A bound, forward 1, B bound, forward 2, unbound, forward 3, one synchronisation --
    A holds the maps of forward 1, B those of forward 2, and forward 3 wrote neither."""
    spec, params, _ = make_case('S16-j17')
    eng = Engine(spec, params, 'f16', max_batch=2, device=cuda)
    x1 = torch.from_numpy(synth.make_images(2, spec.proc_side, seed=9)).to(cuda)
    x2 = torch.from_numpy(synth.make_images(1, spec.proc_side, seed=10)).to(cuda)
    want1, want2 = buffers(eng, 2, cuda), buffers(eng, 1, cuda)
    eng.forward(x1, **want1)
    eng.forward(x2, **want2)
    a, b = buffers(eng, 2, cuda), buffers(eng, 2, cuda)
    nb = lib.metro_plan_heatmaps_scratch_bytes(eng._plan, 2)
    scratch = torch.empty(nb, dtype=torch.uint8, device=cuda)
    poses = torch.empty((2, spec.skeleton.n_out, 3), device=cuda)
    stream = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    fwd = lambda x: check(lib.metro_forward(eng._plan, H.ptr(x), x.shape[0], H.ptr(poses), H.ptr(eng._ws), stream), 'metro_forward')
    torch.cuda.synchronize()
    check(lib.metro_plan_bind_heatmaps(eng._plan, H.ptr(a['heat_xy']), H.ptr(a['heat_z']), H.ptr(scratch), 2), 'bind')
    fwd(x1)
    check(lib.metro_plan_bind_heatmaps(eng._plan, H.ptr(b['heat_xy']), H.ptr(b['heat_z']), H.ptr(scratch), 2), 'bind')
    fwd(x2)
    check(lib.metro_plan_bind_heatmaps(eng._plan, None, None, None, 0), 'unbind')
    fwd(x1)
    torch.cuda.synchronize()
    assert torch.equal(a['heat_xy'], want1['heat_xy']) and torch.equal(a['heat_z'], want1['heat_z'])
    assert torch.equal(b['heat_xy'][:1], want2['heat_xy']) and torch.equal(b['heat_z'][:1], want2['heat_z'])
    assert torch.isnan(b['heat_xy'][1:]).all() and torch.isnan(b['heat_z'][1:]).all()          # rows n .. max_n - 1 are not touched
    assert torch.equal(poses, want1['out'])
    eng.close()


def test_bound_forward_on_a_side_stream(cuda):
    """tests/stream_harness.py snapshots an entry's ARGUMENTS (and regions of its scratch arguments): buffers bound to the plan are
    neither, so the harness cannot hold them unedited.  What is held here: a bound forward enqueued on a non-blocking side stream
    while the default stream is busy gives the bits of the same call on the default stream, after the side stream alone is
    synchronised."""
    spec, params, _ = make_case('S16-j17')
    eng = Engine(spec, params, 'f16', max_batch=2, device=cuda)
    x = torch.from_numpy(synth.make_images(2, spec.proc_side, seed=11)).to(cuda)
    want = buffers(eng, 2, cuda)
    eng.forward(x, **want)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=cuda)
    got = buffers(eng, 2, cuda)
    torch.cuda.synchronize()
    busy = torch.empty((4096, 4096), device=cuda)
    for _ in range(8):
        busy = torch.mm(busy.fill_(1e-3), busy)             # the default stream has work queued behind which nothing of the call may wait
    with torch.cuda.stream(side):
        eng.forward(x, **got)
    side.synchronize()
    for k in want:
        assert torch.equal(got[k], want[k]), k
    torch.cuda.synchronize()
    eng.close()


@pytest.mark.parametrize('precision', ('f16', 'f32m'))
def test_nonfinite_logits_poison_their_joint_only(cuda, precision):
    """A NaN bias on one logits channel makes every logit of that channel NaN: both outputs' rows of its joint are NaN in
    every crop, every other joint keeps the bits of the clean model (its logits are the same numbers), and the poses, the
    statistics, the status words and NonFiniteError are the unbound call's.  f16: the one-launch head's logits; f32m: the
    workspace's."""
    spec, params, _ = make_case('S16-j17')
    nj, bad_joint = spec.skeleton.n_head, 2
    x = torch.from_numpy(synth.make_images(2, spec.proc_side, seed=12)).to(cuda)
    eng = Engine(spec, params, precision, max_batch=2, device=cuda)
    clean = buffers(eng, 2, cuda)
    eng.forward(x, **clean)
    torch.cuda.synchronize()
    eng.close()
    poisoned = dict(params)
    bias = params['MainPart/resnet_v2_50/logits/biases'].copy()
    bias[1 * nj + bad_joint] = np.nan
    poisoned['MainPart/resnet_v2_50/logits/biases'] = bias
    eng = Engine(spec, poisoned, precision, max_batch=2, device=cuda)
    b, u = buffers(eng, 2, cuda), buffers(eng, 2, cuda)
    eng.forward(x, **b)
    words = eng.status_words(2).clone()
    with pytest.raises(_lib.NonFiniteError):
        eng.check_finite(2)
    eng.forward(x, **{k: u[k] for k in ('out', 'coords01', 'cov01', 'peak')})
    assert words.tolist() == [1, 1] and torch.equal(eng.status_words(2), words)
    rows = torch.tensor([p == bad_joint for p in spec.skeleton.permutation], device=cuda)
    assert rows.any() and not rows.all()
    assert torch.isnan(b['heat_xy'][:, rows]).all() and torch.isnan(b['heat_z'][:, rows]).all()
    assert torch.equal(b['heat_xy'][:, ~rows], clean['heat_xy'][:, ~rows]) and torch.equal(b['heat_z'][:, ~rows], clean['heat_z'][:, ~rows])
    for k in ('out', 'coords01', 'cov01', 'peak'):
        assert torch.equal(b[k].nan_to_num(nan=-7.0), u[k].nan_to_num(nan=-7.0)), k
    eng.close()


def test_f64_whole_call_against_the_oracle(cuda):
    """Precision 'f64' end to end on a committed golden toy case: the restatement applied to the fp64 ORACLE's logits."""
    spec, params, images, oracle_logits = golden_case()
    eng = Engine(spec, params, 'f64', max_batch=len(images), device=cuda)
    b = buffers(eng, len(images), cuda)
    eng.forward(torch.from_numpy(images).to(cuda), **b)
    ref = HR.marginals(oracle_logits, spec.skeleton.n_head, spec.depth, list(spec.skeleton.permutation))
    HR.check(b['heat_xy'].cpu().numpy(), b['heat_z'].cpu().numpy(), ref[0], ref[1], 'gpu/f64/golden-oracle',
             spec.heatmap_side ** 2 * spec.depth, GOLDEN)
    eng.close()


def test_estimate_pose_returns_the_heatmaps(cuda, tmp_path):
    from metro_pose3d_amd import inference as INF, save_model
    spec, params, _ = make_case('S16-j17')
    path = str(tmp_path / 'm.npz')
    save_model(path, spec, params)
    x = torch.from_numpy(synth.make_images(3, spec.proc_side, seed=13)).to(cuda)
    plain = INF.estimate_pose(x, path)
    poses, edges, names, heat = INF.estimate_pose(x, path, return_heatmaps=True)
    both = INF.estimate_pose(x, path, return_uncertainty=True, return_heatmaps=True)
    unc = INF.estimate_pose(x, path, return_uncertainty=True)
    assert len(plain) == 3 and len(both) == 5 and isinstance(heat, INF.Heatmaps) and isinstance(both[4], INF.Heatmaps)
    assert torch.equal(poses, plain[0]) and torch.equal(both[0], plain[0])
    assert torch.equal(both[3].covariance, unc[3].covariance) and torch.equal(both[3].peak, unc[3].peak)
    assert torch.equal(both[4].xy, heat.xy) and torch.equal(both[4].z, heat.z)
    eng = Engine(spec, params, 'f16', max_batch=8, device=cuda)
    b = buffers(eng, 3, cuda)
    eng.forward(x, **b)
    assert heat.xy.shape == eng.heat_shapes(3)[0] and torch.equal(heat.xy, b['heat_xy']) and torch.equal(heat.z, b['heat_z'])
    out = str(tmp_path / 'heat.npz')
    img = str(tmp_path / 'img.npy')
    np.save(img, x[0].cpu().numpy())
    INF.main(['--model-path', path, '--image', img, '--heatmaps', out])
    saved = np.load(out)
    assert np.array_equal(saved['xy'], heat.xy[:1].cpu().numpy()) and np.array_equal(saved['z'], heat.z[:1].cpu().numpy())
    eng.close()
    INF.clear_cache()
