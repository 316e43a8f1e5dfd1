"""Per-joint heat-map posterior under a Gaussian prior on the MI355X: toy-width synthetic models (base_width 16) through
Engine.forward_posterior, held to the fp64 restatement (tests/heat_posterior_ref.py) of the logits of the SAME forward at the same
n, read through the layer dump (forward_upto), in all four precisions and at every head shape at which the kernel takes another
path: a volume of 32 voxels (S = 2), an odd side with 53 joints (S = 7), volumes staged whole in LDS (S = 16; 17 and 19 joints),
a volume read from memory three times (S = 64), 1, 2 and 65 crops, more crops than one bound forward takes (heat_chunk).  The
prior rows cycle over (crop + joint) through four kinds: a random positive definite precision, a zero one (log_evidence exactly
0), one that knows nothing along z, and a prior far outside the volume (log_evidence about -1e3, finite).

Tolerances: profiles/heat_posterior_parity.json records the worst deviation per precision and head (log_evidence absolute, peak'
in probability, coords01' in grid steps, cov01' in units of one voxel's variance; tools/heat_posterior_parity.py runs
gpu_deviations() below); the tests assert FOUR times those figures (heat_posterior_ref.gate)."""
import ctypes as C

import numpy as np
import pytest
import torch

from metro_pose3d_amd import ModelSpec, _lib, synth
from metro_pose3d_amd._lib import check
from metro_pose3d_amd.engine import Engine
from tests import helpers as H, heat_posterior_ref as PR
from tests.test_gpu_heat_marginals import HEAT_IDS
from tests.test_gpu_heat_modes import MODES_IDS
from tests.test_heat_posterior import POST_IDS

pytestmark = pytest.mark.gpu

PRECISIONS = ('f16', 'f32', 'f32m', 'f64')
# id -> (stride, proc_side, dataset, depth, the crops per call)
HEADS = {
    'S2': (32, 64, 'h36m', 8, (1, 2, 65)),
    'S7-j53': (32, 224, 'merged', 8, (2,)),
    'S16-j17': (16, 256, 'h36m', 8, (1, 2)),
    'S16-j19': (16, 256, 'many19', 8, (2,)),
    'S64': (4, 256, 'h36m', 8, (1,)),
}
PLAIN = ('out', 'coords01', 'cov01', 'peak')
KINDS = ('psd', 'zero', 'singular-z', 'far')
MODES_KR = (2, 1)


def make_case(head, seed=1):
    stride, side, dataset, depth, ns = HEADS[head]
    spec = ModelSpec(50, stride, dataset, depth=depth, proc_side=side, base_width=16)
    params = synth.make_params(50, spec.n_head_channels, 16, seed=seed, logit_gain=synth.logit_gain_for(50, stride, 16))
    return spec, params, ns


def row_kinds(n, nj):
    """int [n, nj]: the index into KINDS of every prior row."""
    return (np.arange(n)[:, None] + np.arange(nj)[None, :]) % len(KINDS)


def make_prior(n, nj, cuda, seed=3):
    """Prior rows fp32 [n, nj, 9] on the device, the kind of row (i, r) being KINDS[(i + r) % 4]."""
    rng = np.random.default_rng([seed, n, nj])
    mu = rng.uniform(-0.2, 1.2, (n, nj, 3))
    a = rng.standard_normal((n, nj, 3, 3))
    lam = np.einsum('...ab,...cb->...ac', a, a) * 40.0
    kind = row_kinds(n, nj)
    lam[kind == 1] = 0.0
    z = kind == 2
    lam[z, 2, :] = 0.0
    lam[z, :, 2] = 0.0
    mu[kind == 3] = (3.0, -2.0, 0.5)
    lam[kind == 3] = np.diag([200.0, 200.0, 0.0])
    return torch.from_numpy(PR.prior_rows(mu, lam).astype(np.float32)).to(cuda)


def buffers(eng, n, cuda, heat=False):
    sk = eng.spec.skeleton
    f32 = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=cuda)
    b = dict(out=f32(n, sk.n_out, 3), coords01=f32(n, sk.n_head, 3), cov01=f32(n, sk.n_head, 6), peak=f32(n, sk.n_head))
    if heat:
        xy_shape, z_shape = eng.heat_shapes(n)
        b.update(heat_xy=f32(*xy_shape), heat_z=f32(*z_shape))
    return b


def same(a, b):
    """Bit equality of two float tensors (NaN rows included)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run_bound(eng, x, prior, cuda):
    """-> (the bound call's tensors with 'post', the unbound call's, the restatement of the same forward's dumped logits).  With
    eng.heat_chunk set the bound call is made of forwards of at most that many crops: the unbound call and the dump are made of
    the same."""
    n, spec = x.shape[0], eng.spec
    b = buffers(eng, n, cuda)
    _, b['post'] = eng.forward_posterior(x, prior, **b)
    u = buffers(eng, n, cuda)
    step = eng.heat_chunk or n
    dumps = []
    for i in range(0, n, step):
        eng.forward(x[i:i + step], **{key: u[key][i:i + step] for key in PLAIN})
        dumps.append(eng.forward_upto(x[i:i + step], len(eng.layer_infos()) - 2).cpu().numpy())
    ref = PR.posterior(np.concatenate(dumps), spec.skeleton.n_head, spec.depth, list(spec.skeleton.permutation), prior.cpu().numpy())
    return b, u, ref


def hold(b, u, ref, spec, key, what):
    post = b['post'].cpu().numpy()
    assert np.isfinite(ref).all(), what
    PR.check(post, ref, spec.heatmap_side, spec.depth, PR.gate(key), key, what)
    kind = row_kinds(*post.shape[:2])
    assert (post[kind == 1][:, 0] == 0.0).all(), (what, 'a zero precision: log_evidence exactly 0')
    assert (post[kind == 3][:, 0] < -700).all(), (what, 'a prior far outside the volume')
    for k in PLAIN:
        assert torch.equal(b[k], u[k]), (what, k)


def gpu_deviations(cuda):
    """{key: {measure: worst}} of every comparison of this file: what tools/heat_posterior_parity.py records."""
    out = {}
    for precision in PRECISIONS:
        for head in HEADS:
            spec, params, ns = make_case(head)
            eng = Engine(spec, params, precision, max_batch=max(ns), device=cuda)
            worst = dict.fromkeys(PR.MEASURES, 0.0)
            inputs = [torch.from_numpy(synth.make_images(n, spec.proc_side, seed=7)).to(cuda) for n in ns]
            if head == UINT8_HEAD and precision in UINT8_PRECISIONS:
                inputs.append(uint8_crops(spec, cuda))
            for x in inputs:
                for chunk in ((None, 32) if x.shape[0] > 32 else (None,)):
                    eng.heat_chunk = chunk
                    b, _, ref = run_bound(eng, x, make_prior(x.shape[0], spec.skeleton.n_out, cuda), cuda)
                    dev = PR.deviation(b['post'].cpu().numpy(), ref, spec.heatmap_side, spec.depth)
                    worst = {m: max(worst[m], dev[m]) for m in worst}
                    print(f'gpu/{precision}/{head} n{x.shape[0]} chunk {chunk}: ' + ' '.join(f'{m} {dev[m]:.3e}' for m in dev), flush=True)
            eng.close()
            out[f'gpu/{precision}/{head}'] = worst
    return out


UINT8_HEAD, UINT8_PRECISIONS = 'S16-j17', ('f16', 'f32m')


def uint8_crops(spec, cuda):
    return torch.from_numpy(np.round(synth.make_images(2, spec.proc_side, seed=8) * 255).astype(np.uint8)).to(cuda)


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('head', list(HEADS))
def test_bound_forward_against_the_logits_of_the_same_forward(cuda, lib, head, precision):
    spec, params, ns = make_case(head)
    eng = Engine(spec, params, precision, max_batch=max(ns), device=cuda)
    key = f'gpu/{precision}/{head}'
    nj = spec.skeleton.n_out
    for n in ns:
        x = torch.from_numpy(synth.make_images(n, spec.proc_side, seed=7)).to(cuda)
        for chunk in ((None, 32) if n > 32 else (None,)):          # 65 crops: one bound forward, and 32 + 32 + 1
            eng.heat_chunk = chunk
            b, u, ref = run_bound(eng, x, make_prior(n, nj, cuda), cuda)
            hold(b, u, ref, spec, key, f'n{n} chunk {chunk}')
            if chunk is not None:                                   # the status words are the call's, not the last chunk's
                assert eng.status_words(n).shape == (n,) and not eng.status_words(n).any()
    eng.heat_chunk = None
    # prior, modes and heat-maps bound together: each output has the bits it has when bound alone
    n = ns[-1]
    x = torch.from_numpy(synth.make_images(n, spec.proc_side, seed=7)).to(cuda)
    prior = make_prior(n, nj, cuda)
    k, radius = MODES_KR
    alone = buffers(eng, n, cuda)
    _, alone['post'] = eng.forward_posterior(x, prior, **alone)
    modes = buffers(eng, n, cuda)
    _, modes['voxel'], modes['stats'] = eng.forward_modes(x, k, radius, **modes)
    heat = buffers(eng, n, cuda, heat=True)
    eng.forward(x, **heat)
    # what the forward enqueues: unbound, the plan's own list; bound, the posterior launch behind it
    plan_ids = ' & '.join(eng.layer_kernels(n))
    check(lib.metro_kernel_notes(1), 'notes')
    eng.forward(x)
    unbound_ids = lib.metro_last_kernel_id().decode()
    check(lib.metro_kernel_notes(1), 'notes')
    eng.forward_posterior(x, prior)
    bound_ids = lib.metro_last_kernel_id().decode()
    both = buffers(eng, n, cuda, heat=True)
    both['post'] = torch.full((n, nj, PR.STATS), -7.0, device=cuda)
    scratch = torch.empty(lib.metro_plan_prior_scratch_bytes(eng._plan, n), dtype=torch.uint8, device=cuda)
    check(lib.metro_plan_bind_prior(eng._plan, H.ptr(prior), H.ptr(both['post']), H.ptr(scratch), n), 'bind')
    try:
        check(lib.metro_kernel_notes(1), 'notes')
        _, both['voxel'], both['stats'] = eng.forward_modes(x, k, radius, **{key_: both[key_] for key_ in PLAIN + ('heat_xy', 'heat_z')})
        all_ids = lib.metro_last_kernel_id().decode()
    finally:
        check(lib.metro_kernel_notes(0), 'notes')
        check(lib.metro_plan_bind_prior(eng._plan, None, None, None, 0), 'unbind')
    assert unbound_ids == plan_ids, (unbound_ids, plan_ids)
    assert bound_ids == plan_ids + ' & ' + POST_IDS[precision], bound_ids
    # (that call also asked for cov01 and peak: its head and finalize launches are the MOMENTS instantiations)
    assert all_ids.endswith(' & '.join(('', HEAT_IDS[precision], MODES_IDS[precision], POST_IDS[precision]))), all_ids[-300:]
    assert all_ids.count(' & ') == plan_ids.count(' & ') + 5, all_ids
    assert same(both['post'], alone['post'])
    assert torch.equal(both['voxel'], modes['voxel']) and same(both['stats'], modes['stats'])
    for key_ in PLAIN + ('heat_xy', 'heat_z'):
        assert torch.equal(both[key_], heat[key_]), key_
    eng.close()


@pytest.mark.parametrize('precision', UINT8_PRECISIONS)
def test_uint8_crops(cuda, precision):
    """f16 reads the bytes in its first kernel (metro_forward_u8), the parity precisions expand them first: both bound."""
    spec, params, _ = make_case(UINT8_HEAD)
    eng = Engine(spec, params, precision, max_batch=2, device=cuda)
    b, u, ref = run_bound(eng, uint8_crops(spec, cuda), make_prior(2, spec.skeleton.n_out, cuda), cuda)
    hold(b, u, ref, spec, f'gpu/{precision}/{UINT8_HEAD}', 'uint8')
    eng.close()


def raw_output(eng, n, cuda):
    return torch.full((n, eng.spec.skeleton.n_out, PR.STATS), -7.0, dtype=torch.float32, device=cuda)


def test_rebinding_and_unbinding_between_enqueues(cuda, lib):
    """Binding is host state read at enqueue: A bound, forward 1, B bound (another prior), forward 2, unbound, forward 3, one
    synchronisation -- A holds the posterior of forward 1, B that of forward 2, and forward 3 wrote neither."""
    spec, params, _ = make_case('S16-j17')
    eng = Engine(spec, params, 'f16', max_batch=2, device=cuda)
    nj = spec.skeleton.n_out
    x1 = torch.from_numpy(synth.make_images(2, spec.proc_side, seed=9)).to(cuda)
    x2 = torch.from_numpy(synth.make_images(1, spec.proc_side, seed=10)).to(cuda)
    p1, p2 = make_prior(2, nj, cuda, seed=4), make_prior(2, nj, cuda, seed=5)
    want_pose, want1 = eng.forward_posterior(x1, p1)
    _, want2 = eng.forward_posterior(x2, p2[:1])
    a, b = raw_output(eng, 2, cuda), raw_output(eng, 2, cuda)
    scratch = torch.empty(lib.metro_plan_prior_scratch_bytes(eng._plan, 2), dtype=torch.uint8, device=cuda)
    poses = torch.empty((2, nj, 3), device=cuda)
    stream = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    fwd = lambda x: check(lib.metro_forward(eng._plan, H.ptr(x), x.shape[0], H.ptr(poses), H.ptr(eng._ws), stream), 'metro_forward')
    torch.cuda.synchronize()
    check(lib.metro_plan_bind_prior(eng._plan, H.ptr(p1), H.ptr(a), H.ptr(scratch), 2), 'bind')
    fwd(x1)
    check(lib.metro_plan_bind_prior(eng._plan, H.ptr(p2), H.ptr(b), H.ptr(scratch), 2), 'bind')
    fwd(x2)
    check(lib.metro_plan_bind_prior(eng._plan, None, None, None, 0), 'unbind')
    fwd(x1)
    torch.cuda.synchronize()
    assert same(a, want1)
    assert same(b[:1], want2)
    assert (b[1:] == -7).all()                                            # rows n .. max_n - 1 are not touched
    assert torch.equal(poses, want_pose)
    eng.close()


def test_more_crops_than_bound_are_refused_before_any_launch(cuda, lib):
    spec, params, _ = make_case('S16-j17')
    eng = Engine(spec, params, 'f16', max_batch=2, device=cuda)
    x = torch.from_numpy(synth.make_images(2, spec.proc_side, seed=9)).to(cuda)
    post, prior = raw_output(eng, 1, cuda), make_prior(1, spec.skeleton.n_out, cuda)
    scratch = torch.empty(lib.metro_plan_prior_scratch_bytes(eng._plan, 1), dtype=torch.uint8, device=cuda)
    poses = torch.full((2, spec.skeleton.n_out, 3), -7.0, device=cuda)
    stream = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    check(lib.metro_plan_bind_prior(eng._plan, H.ptr(prior), H.ptr(post), H.ptr(scratch), 1), 'bind')
    try:
        check(lib.metro_kernel_notes(1), 'notes')
        assert lib.metro_forward(eng._plan, H.ptr(x), 2, H.ptr(poses), H.ptr(eng._ws), stream) == -1
        assert b'bound prior buffers' in lib.metro_last_error() and lib.metro_last_kernel_id() == b''
    finally:
        check(lib.metro_kernel_notes(0), 'notes')
        check(lib.metro_plan_bind_prior(eng._plan, None, None, None, 0), 'unbind')
    torch.cuda.synchronize()
    assert (poses == -7).all() and (post == -7).all()
    eng.close()


def test_metro_forward_with_a_prior_bound_keeps_to_a_side_stream(cuda, lib):
    """The protocol of tests/stream_harness.py on metro_forward with a prior bound (a chain: the bound buffers are no arguments of
    the entry): on a non-blocking side stream, behind the delay, the call returns while the delay runs and poses and post have the
    bits of the default-stream run."""
    from tests import stream_harness as SH
    spec, params, _ = make_case('S16-j17')
    eng = Engine(spec, params, 'f16', max_batch=2, device=cuda)
    scratch = torch.empty(lib.metro_plan_prior_scratch_bytes(eng._plan, 2), dtype=torch.uint8, device=cuda)
    prior = make_prior(2, spec.skeleton.n_out, cuda)

    def fn(images):
        post = raw_output(eng, 2, cuda)
        poses = torch.empty((2, spec.skeleton.n_out, 3), device=cuda)
        check(lib.metro_plan_bind_prior(eng._plan, H.ptr(prior), H.ptr(post), H.ptr(scratch), 2), 'bind')
        try:
            check(lib.metro_forward(eng._plan, H.ptr(images), 2, H.ptr(poses), H.ptr(eng._ws),
                                    C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)), 'metro_forward')
        finally:
            check(lib.metro_plan_bind_prior(eng._plan, None, None, None, 0), 'unbind')
        return poses, post
    a, b = (torch.from_numpy(synth.make_images(2, spec.proc_side, seed=s)).to(cuda) for s in (11, 12))
    SH.verdict(SH.Chain(fn, [a], [b]), cuda, what='metro_forward, prior bound', asynchronous=True, busy=False).require_ok()
    eng.close()


def test_nonfinite_logits_poison_their_joint_only(cuda):
    """A NaN bias on one logits channel: all 11 values of its joint are NaN in every crop, every other joint keeps the bits of the
    clean model, and poses, statistics and status words are the unbound call's.  A NaN in a prior row does the same to its row."""
    spec, params, _ = make_case('S16-j17')
    nj, bad_joint = spec.skeleton.n_head, 2
    x = torch.from_numpy(synth.make_images(2, spec.proc_side, seed=12)).to(cuda)
    prior = make_prior(2, spec.skeleton.n_out, cuda)
    eng = Engine(spec, params, 'f16', max_batch=2, device=cuda)
    _, clean = eng.forward_posterior(x, prior)
    bad_prior = prior.clone()
    bad_prior[1, 4, 7] = float('nan')
    _, got = eng.forward_posterior(x, bad_prior)
    keep = torch.ones((2, spec.skeleton.n_out), dtype=torch.bool, device=cuda)
    keep[1, 4] = False
    assert torch.isnan(got[1, 4]).all() and same(got[keep], clean[keep]) and not eng.status_words(2).any()
    torch.cuda.synchronize()
    eng.close()
    poisoned = dict(params)
    bias = params['MainPart/resnet_v2_50/logits/biases'].copy()
    bias[1 * nj + bad_joint] = np.nan
    poisoned['MainPart/resnet_v2_50/logits/biases'] = bias
    eng = Engine(spec, poisoned, 'f16', max_batch=2, device=cuda)
    b, u = buffers(eng, 2, cuda), buffers(eng, 2, cuda)
    _, post = eng.forward_posterior(x, prior, **b)
    words = eng.status_words(2).clone()
    eng.forward(x, **u)
    assert words.tolist() == [1, 1] and torch.equal(eng.status_words(2), words)
    rows = torch.tensor([p == bad_joint for p in spec.skeleton.permutation], device=cuda)
    assert rows.any() and not rows.all()
    assert torch.isnan(post[:, rows]).all()
    assert same(post[:, ~rows], clean[:, ~rows])
    for key in PLAIN:
        assert torch.equal(b[key].nan_to_num(nan=-7.0), u[key].nan_to_num(nan=-7.0)), key
    eng.close()


def test_forward_posterior_in_chunks_equals_the_chunks_done_by_hand(cuda):
    spec, params, _ = make_case('S16-j17')
    eng = Engine(spec, params, 'f16', max_batch=3, device=cuda)
    x = torch.from_numpy(synth.make_images(3, spec.proc_side, seed=14)).to(cuda)
    prior = make_prior(3, spec.skeleton.n_out, cuda)
    by_hand = [eng.forward_posterior(x[i:i + 1], prior[i:i + 1]) for i in range(3)]
    eng.heat_chunk = 1
    poses, post = eng.forward_posterior(x, prior)
    eng.heat_chunk = None
    for i, want in enumerate(zip(*by_hand)):
        assert same((poses, post)[i], torch.cat(want)), i
    assert eng.status_words(3).shape == (3,) and not eng.status_words(3).any()
    eng.close()


def test_estimate_pose_posterior_is_forward_posterior_and_the_metric_conversion(cuda, tmp_path):
    from metro_pose3d_amd import inference as INF, save_model
    spec, params, _ = make_case('S16-j17')
    path = str(tmp_path / 'm.npz')
    save_model(path, spec, params)
    nj = spec.skeleton.n_out
    x = torch.from_numpy(synth.make_images(3, spec.proc_side, seed=13)).to(cuda)
    rng = np.random.default_rng(15)
    pos_mm = rng.uniform(200, 2000, (3, nj, 3))
    lam_mm = np.broadcast_to(np.diag([1 / 150.0 ** 2, 1 / 150.0 ** 2, 0.0]), (3, nj, 3, 3)).copy()
    lam_mm[:, ::2] = 0.0                                                     # every second joint: nothing known
    plain = INF.estimate_pose(x, path, return_uncertainty=True, return_heatmaps=True)
    res = INF.estimate_pose_posterior(x, path, pos_mm, lam_mm, return_uncertainty=True, return_heatmaps=True)
    short = INF.estimate_pose_posterior(x, path, torch.from_numpy(pos_mm).to(cuda), torch.from_numpy(lam_mm).to(cuda))
    assert len(res) == 6 and len(short) == 4 and isinstance(res[-1], INF.Posterior) and isinstance(short[-1], INF.Posterior)
    assert torch.equal(res[0], plain[0]) and torch.equal(short[0], plain[0])
    assert np.array_equal(res[1], plain[1]) and list(res[2]) == list(plain[2])
    assert torch.equal(res[3].covariance, plain[3].covariance) and torch.equal(res[3].peak, plain[3].peak)
    assert torch.equal(res[4].xy, plain[4].xy) and torch.equal(res[4].z, plain[4].z)
    for a, b in zip(res[-1], short[-1]):
        assert same(a, b)
    # the composition, written out in torch: heatmap_to_metric of the posterior mean, minus that of the posterior root
    eng = Engine(spec, params, 'f16', max_batch=8, device=cuda)
    prior = INF.pose_prior(spec, pos_mm, lam_mm).to(cuda)
    _, post = eng.forward_posterior(x, prior)
    last = spec.proc_side - 1
    lrc, half, box, side = last - last % spec.stride - 1, spec.stride // 2, spec.box_size_mm, spec.proc_side
    mm = lambda c: torch.cat([(c[..., :2] * lrc + half) * box / side, c[..., 2:] * box], -1)
    at = mm(post[..., 2:5].double())
    root = list(spec.skeleton.permutation).index(spec.skeleton.n_head - 1)
    m = res[-1]
    assert torch.allclose(m.positions.double(), at, rtol=1e-7, atol=0) and same(m.log_evidence, post[..., 0]) and same(m.peak, post[..., 1])
    assert torch.allclose(m.poses.double(), at - at[:, root:root + 1], rtol=0, atol=1e-3)
    s = torch.tensor([lrc * box / side, lrc * box / side, box], dtype=torch.float64, device=cuda)
    idx = torch.tensor([[5, 8, 9], [8, 6, 10], [9, 10, 7]], device=cuda)
    assert same(m.covariance, (post.double()[..., idx] * (s[:, None] * s[None, :])).float())
    # nothing known: the plain pose, position for position, and no evidence against it
    assert (m.log_evidence[:, ::2] == 0).all() and (m.log_evidence[:, 1::2] < 0).all()
    img, npz = str(tmp_path / 'img.npy'), str(tmp_path / 'prior.npz')
    np.save(img, x[0].cpu().numpy())
    np.savez(npz, positions=pos_mm[0], precision=lam_mm[0])
    INF.main(['--model-path', path, '--image', img, '--prior', npz])
    eng.close()
    INF.clear_cache()
