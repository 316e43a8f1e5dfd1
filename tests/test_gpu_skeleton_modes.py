"""The choice among heat-map modes by bone lengths on the MI355X: toy-width synthetic models (base_width 16).
  1  Hand-filled mode buffers (the CPU cases of tests/skeleton_modes_ref.py) bound to a plan with metro_plan_bind_skeleton_modes
     -- the modes binding is not required -- at 1, 2 and 65 rows on f16 and f64 plans: the one launch of the wave-sized team.
  2  The forward's own modes (Engine.forward_skeleton_modes): S = 2 with radius 0 and S = 16 with radius 1; 17, 19 and 53 head
     joints; 1 to 65 crops, uint8 crops, a side stream; against the restatement fed with the voxel / stats the same forward wrote.
  3  The Python layer: rebinding between enqueues, estimate_pose_skeleton as the composition written out.

Bounds (skeleton_modes_ref.compare): choice exact; prob within 1e-9 and both logs within 1e-9 max(1, |value|) of the restatement.
The device's outputs are fp32, the kernel's one rounding of its fp64 value: that rounding's half ulp (2^-24 relative) is added,
which is the format's precision, not the code's.  coords01_sel exact.  In (2) a joint whose best two max-marginals are closer than
1e-6 in the restatement is left out of the choice comparison only; there may be at most one in a thousand per case."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from metro_pose3d_amd import ModelSpec, _lib, synth
from metro_pose3d_amd import heads as MH
from metro_pose3d_amd._lib import check
from metro_pose3d_amd.engine import Engine
from metro_pose3d_amd.joints import skeleton
from tests import helpers as H, skeleton_modes_ref as SR

pytestmark = pytest.mark.gpu

PLAIN = ('out', 'coords01', 'cov01', 'peak')
# id -> (stride, proc_side, dataset, radius)
HEADS = {
    'S2-j17': (32, 64, 'h36m', 0),
    'S16-j17': (16, 256, 'h36m', 1),
    'S2-j19': (32, 64, 'many19', 0),
    'S16-j53': (16, 256, 'merged', 1),
}


def make_model(head, seed=1):
    stride, side, dataset, radius = HEADS[head]
    spec = ModelSpec(50, stride, dataset, proc_side=side, base_width=16)
    params = synth.make_params(50, spec.n_head_channels, 16, seed=seed, logit_gain=synth.logit_gain_for(50, stride, 16))
    return spec, params, radius


def metric_scale(spec):
    from metro_pose3d_amd.inference import _metric_map
    return _metric_map(spec)[0]


def images(spec, n, cuda, seed=7):
    return torch.from_numpy(synth.make_images(n, spec.proc_side, seed=seed)).to(cuda)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- 1: hand-filled mode buffers ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def hand_cases(dataset, rows):
    """The CPU cases at this dataset's output joints, each with its restatement (computed once, shared by the precisions): the
    skeleton's own edges, a chain, a star, a random forest, no edge; K = 1, 2, 3 at every row count, K = 8 at 1 and 2 rows."""
    sk = skeleton(dataset)
    nj = sk.n_out
    own = [tuple(e) for e in sk.edges]
    rng = np.random.default_rng([nj, rows])
    out = []
    for name, k, edges in (('own-k2', 2, own), ('own-k8', 8, own), ('own-k1', 1, own), ('chain-k2', 2, SR.chain(nj)), ('star-k8', 8, SR.star(nj)),
                           ('forest-k3', 3, SR.random_tree(rng, nj, nj // 2)), ('no-edge-k2', 2, [])):
        if k == 8 and rows > 2:
            continue
        case = SR.make_case([len(name), rows, nj, k], rows, nj, k, edges, n_head=sk.n_head)
        case['perm'] = list(sk.permutation)
        out.append((name, case, SR.infer(case['voxel'], case['stats'], case['lengths'], case['edges'], SR.SCALE)))
    return out


def run_hand(eng, lib, case, x, cuda, max_n=None):
    """The case's buffers on the device, bound without the modes binding; one metro_forward_coords01."""
    spec, rows, k = eng.spec, case['rows'], case['k']
    sk = spec.skeleton
    max_n = rows if max_n is None else max_n
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(cuda)
    voxel, stats, lengths = dev(case['voxel'], np.int32), dev(case['stats'], np.float32), dev(case['lengths'], np.float64)
    if lengths.numel() == 0:
        lengths = torch.zeros(1, dtype=torch.float64, device=cuda)
    prob = torch.full((max_n, sk.n_out, k), -7.0, device=cuda)
    info = torch.full((max_n, sk.n_out, 2), -7.0, device=cuda)
    choice = torch.full((max_n, sk.n_out), -7, dtype=torch.int32, device=cuda)
    sel = torch.full((max_n, sk.n_head, 3), -7.0, device=cuda)
    poses, coords01 = torch.empty((rows, sk.n_out, 3), device=cuda), torch.empty((rows, sk.n_head, 3), device=cuda)
    edges = np.ascontiguousarray(np.asarray(case['edges'], np.int32).reshape(-1, 2))
    params = MH.skeleton_mode_params(SR.SCALE)
    stream = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    check(lib.metro_plan_bind_skeleton_modes(eng._plan, H.ptr(voxel), H.ptr(stats), k, H.ptr(lengths),
                                             edges.ctypes.data_as(C.c_void_p) if len(edges) else None, len(edges), C.byref(params),
                                             H.ptr(prob), H.ptr(choice), H.ptr(info), H.ptr(sel), max_n), 'bind')
    try:
        check(lib.metro_forward_coords01(eng._plan, H.ptr(x), rows, H.ptr(poses), H.ptr(coords01), H.ptr(eng._ws), stream), 'forward')
    finally:
        check(lib.metro_plan_bind_skeleton_modes(eng._plan, None, None, 0, None, None, 0, None, None, None, None, None, 0), 'unbind')
    torch.cuda.synchronize()
    return dict(prob=prob, choice=choice, info=info, sel=sel, poses=poses, coords01=coords01)


def hand_deviations(cuda, lib, precision, dataset, rows_list=(1, 2, 65)):
    """{case: (prob, logs)}: the worst deviations of the hand-filled cases from the restatement (tools/skeleton_modes_parity.py
    records them); every case is held to compare()'s bounds on the way."""
    spec = ModelSpec(50, 32, dataset, proc_side=64, base_width=16)
    params = synth.make_params(50, spec.n_head_channels, 16, seed=1, logit_gain=synth.logit_gain_for(50, 32, 16))
    eng = Engine(spec, params, precision, max_batch=max(rows_list), device=cuda)
    out = {}
    for rows in rows_list:
        x = images(spec, rows, cuda)
        want_c01 = torch.empty((rows, spec.skeleton.n_head, 3), device=cuda)
        want_pose = eng.forward(x, coords01=want_c01).clone()
        for name, case, ref in hand_cases(dataset, rows):
            got = run_hand(eng, lib, case, x, cuda, max_n=rows + (1 if rows == 2 else 0))
            assert torch.equal(got['poses'], want_pose) and torch.equal(got['coords01'], want_c01), (name, 'the plain outputs keep their bits')
            if rows == 2:                                                          # rows n .. max_n - 1 are not touched
                assert all((got[key][2:] == -7).all() for key in ('prob', 'choice', 'info', 'sel')), name
            cpu = {key: got[key][:rows].cpu().numpy() for key in ('prob', 'choice', 'info', 'sel')}
            dev = SR.compare(cpu, dict(case, coords01=want_c01.cpu().numpy()), ref, f'gpu/{precision}/{dataset}/{name}/rows{rows}', wide=False)
            old = out.get(name, (0.0, 0.0))
            out[name] = (max(old[0], float(dev[0])), max(old[1], float(dev[1])))
    eng.close()
    return out


@pytest.mark.parametrize('precision', ('f16', 'f64'))
@pytest.mark.parametrize('dataset', ('h36m', 'merged'))
def test_hand_filled_modes_bound_without_the_modes_binding(cuda, lib, precision, dataset):
    hand_deviations(cuda, lib, precision, dataset)


# ---- 2: the forward's own modes ----------------------------------------------------------------------------------------------------

def bone_rows(spec, n, cuda, seed=3):
    """Lengths [n, E] for any crops: a spread of plausible bones, one in eight unknown."""
    rng = np.random.default_rng(seed)
    lengths = rng.uniform(80.0, 600.0, (n, len(spec.skeleton.edges)))
    lengths[rng.random(lengths.shape) < 0.125] = np.nan
    return torch.from_numpy(lengths).to(cuda)


def buffers(eng, n, cuda):
    sk = eng.spec.skeleton
    f32 = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=cuda)
    return dict(out=f32(n, sk.n_out, 3), coords01=f32(n, sk.n_head, 3), cov01=f32(n, sk.n_head, 6), peak=f32(n, sk.n_head))


def hold_forward(eng, x, lengths, k, radius, cuda, what):
    spec = eng.spec
    n = x.shape[0]
    b, u = buffers(eng, n, cuda), buffers(eng, n, cuda)
    _, voxel, stats, choice, prob, info, sel = eng.forward_skeleton_modes(x, lengths, k, radius, **b)
    words = eng.status_words(n).clone()
    _, want_voxel, want_stats = eng.forward_modes(x, k, radius, **u)
    assert torch.equal(voxel, want_voxel) and same(stats, want_stats), (what, 'modes')
    assert torch.equal(words, eng.status_words(n)), (what, 'status words')
    for key in PLAIN:
        assert torch.equal(b[key], u[key]), (what, key)
    case = dict(voxel=voxel.cpu().numpy(), stats=stats.cpu().numpy(), lengths=lengths.cpu().numpy(), coords01=b['coords01'].cpu().numpy(),
                edges=[tuple(e) for e in spec.skeleton.edges], perm=list(spec.skeleton.permutation))
    scale = metric_scale(spec)
    ref = SR.infer(case['voxel'], case['stats'], case['lengths'], case['edges'], scale)
    got = dict(prob=prob.cpu().numpy(), choice=choice.cpu().numpy(), info=info.cpu().numpy(), sel=None)
    SR.compare(got, case, ref, what, wide=False, skip_close=True)
    want_sel = SR.select_coords01(case['coords01'], case['stats'], got['choice'], case['perm'])
    assert np.array_equal(sel.cpu().numpy(), want_sel), (what, 'coords01_sel follows the choice')
    return got, ref


@pytest.mark.parametrize('precision', ('f16', 'f64'))
@pytest.mark.parametrize('head', list(HEADS))
def test_forward_skeleton_modes_against_the_modes_of_the_same_forward(cuda, head, precision):
    spec, params, radius = make_model(head)
    ns = (1, 2, 65) if head == 'S2-j17' else (3,)
    eng = Engine(spec, params, precision, max_batch=max(ns), device=cuda)
    for n in ns:
        for chunk in ((None, 32) if n > 32 else (None,)):                           # 65 crops: one bound forward, and 32 + 32 + 1
            eng.heat_chunk = chunk
            hold_forward(eng, images(spec, n, cuda), bone_rows(spec, n, cuda), 2 if n != 2 else 8, radius, cuda,
                         f'gpu/{precision}/{head}/n{n}/chunk{chunk}')
    eng.heat_chunk = None
    eng.close()


@pytest.mark.parametrize('precision', ('f16', 'f32m'))
def test_uint8_crops(cuda, precision):
    spec, params, radius = make_model('S16-j17')
    eng = Engine(spec, params, precision, max_batch=2, device=cuda)
    x = torch.from_numpy(np.round(synth.make_images(2, spec.proc_side, seed=8) * 255).astype(np.uint8)).to(cuda)
    hold_forward(eng, x, bone_rows(spec, 2, cuda), 2, radius, cuda, f'gpu/{precision}/uint8')
    eng.close()


def test_what_a_bound_forward_enqueues(cuda, lib):
    spec, params, radius = make_model('S2-j17')
    eng = Engine(spec, params, 'f16', max_batch=2, device=cuda)
    x = images(spec, 2, cuda)
    plan_ids = ' & '.join(eng.layer_kernels(2))
    check(lib.metro_kernel_notes(1), 'notes')
    eng.forward(x)
    unbound = lib.metro_last_kernel_id().decode()
    check(lib.metro_kernel_notes(1), 'notes')
    eng.forward_skeleton_modes(x, bone_rows(spec, 2, cuda), 2, radius)
    bound = lib.metro_last_kernel_id().decode()
    check(lib.metro_kernel_notes(1), 'notes')
    eng.forward(x)
    after = lib.metro_last_kernel_id().decode()
    check(lib.metro_kernel_notes(0), 'notes')
    assert unbound == plan_ids == after, 'unbound, a forward enqueues exactly the kernels it always did'
    assert bound == plan_ids + ' & heat_modes<acc32,logits32> & skeleton_modes', bound
    eng.close()


def test_metro_forward_with_the_skeleton_bound_keeps_to_a_side_stream(cuda, lib):
    """The protocol of tests/stream_harness.py on metro_forward_coords01 with modes and skeleton bound (a chain: the bound buffers
    are no arguments of the entry)."""
    from tests import stream_harness as SH
    spec, params, radius = make_model('S16-j17')
    sk = spec.skeleton
    eng = Engine(spec, params, 'f16', max_batch=2, device=cuda)
    scratch = torch.empty(lib.metro_plan_modes_scratch_bytes(eng._plan, 2), dtype=torch.uint8, device=cuda)
    lengths = bone_rows(spec, 2, cuda)
    edges = np.ascontiguousarray(sk.edges_array(), np.int32)
    params_c = MH.skeleton_mode_params(metric_scale(spec))

    def fn(x):
        vx = torch.full((2, sk.n_out, 2), -7, dtype=torch.int32, device=cuda)
        st, prob = torch.full((2, sk.n_out, 2, 11), -7.0, device=cuda), torch.full((2, sk.n_out, 2), -7.0, device=cuda)
        choice, info = torch.full((2, sk.n_out), -7, dtype=torch.int32, device=cuda), torch.full((2, sk.n_out, 2), -7.0, device=cuda)
        sel, poses, c01 = (torch.empty(s, device=cuda) for s in ((2, sk.n_head, 3), (2, sk.n_out, 3), (2, sk.n_head, 3)))
        check(lib.metro_plan_bind_modes(eng._plan, H.ptr(vx), H.ptr(st), H.ptr(scratch), 2, 2, radius), 'bind')
        check(lib.metro_plan_bind_skeleton_modes(eng._plan, H.ptr(vx), H.ptr(st), 2, H.ptr(lengths), edges.ctypes.data_as(C.c_void_p), len(edges),
                                                 C.byref(params_c), H.ptr(prob), H.ptr(choice), H.ptr(info), H.ptr(sel), 2), 'bind')
        try:
            check(lib.metro_forward_coords01(eng._plan, H.ptr(x), 2, H.ptr(poses), H.ptr(c01), H.ptr(eng._ws),
                                             C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)), 'metro_forward_coords01')
        finally:
            check(lib.metro_plan_bind_skeleton_modes(eng._plan, None, None, 0, None, None, 0, None, None, None, None, None, 0), 'unbind')
            check(lib.metro_plan_bind_modes(eng._plan, None, None, None, 0, 0, 0), 'unbind')
        return poses, vx, st, prob, choice, info, sel
    a, b = (images(spec, 2, cuda, seed=s) for s in (11, 12))
    SH.verdict(SH.Chain(fn, [a], [b]), cuda, what='metro_forward_coords01, skeleton bound', asynchronous=True, busy=False).require_ok()
    eng.close()


# ---- 3: the Python layer -----------------------------------------------------------------------------------------------------------

def test_rebinding_and_unbinding_between_enqueues(cuda, lib):
    """Binding is host state read at enqueue: A bound, forward 1, B bound (other lengths, edges and sigma), forward 2, unbound,
    forward 3, one synchronisation -- A holds the choice of forward 1, B that of forward 2, and forward 3 wrote neither."""
    spec, params, radius = make_model('S16-j17')
    sk = spec.skeleton
    eng = Engine(spec, params, 'f16', max_batch=2, device=cuda)
    x1, x2 = images(spec, 2, cuda, seed=9), images(spec, 1, cuda, seed=10)
    l1, l2 = bone_rows(spec, 2, cuda, seed=4), bone_rows(spec, 1, cuda, seed=5)[:, :5].contiguous()
    e2 = sk.edges_array()[:5]
    want1 = eng.forward_skeleton_modes(x1, l1, 2, radius)
    want2 = eng.forward_skeleton_modes(x2, l2, 2, radius, edges=e2, sigma_mm=35.0)
    torch.cuda.synchronize()

    def raw(n):
        return dict(vx=torch.full((n, sk.n_out, 2), -7, dtype=torch.int32, device=cuda), st=torch.full((n, sk.n_out, 2, 11), -7.0, device=cuda),
                    prob=torch.full((n, sk.n_out, 2), -7.0, device=cuda), choice=torch.full((n, sk.n_out), -7, dtype=torch.int32, device=cuda),
                    info=torch.full((n, sk.n_out, 2), -7.0, device=cuda), sel=torch.full((n, sk.n_head, 3), -7.0, device=cuda))
    a, b = raw(2), raw(2)
    scratch = torch.empty(lib.metro_plan_modes_scratch_bytes(eng._plan, 2), dtype=torch.uint8, device=cuda)
    poses, c01 = torch.empty((2, sk.n_out, 3), device=cuda), torch.empty((2, sk.n_head, 3), device=cuda)
    stream = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    fwd = lambda x: check(lib.metro_forward_coords01(eng._plan, H.ptr(x), x.shape[0], H.ptr(poses), H.ptr(c01), H.ptr(eng._ws), stream), 'forward')
    scale = metric_scale(spec)

    def bind(t, lengths, edges, sigma):
        e = np.ascontiguousarray(edges, np.int32)
        p = MH.skeleton_mode_params(scale, sigma_mm=sigma)
        check(lib.metro_plan_bind_modes(eng._plan, H.ptr(t['vx']), H.ptr(t['st']), H.ptr(scratch), 2, 2, radius), 'bind')
        check(lib.metro_plan_bind_skeleton_modes(eng._plan, H.ptr(t['vx']), H.ptr(t['st']), 2, H.ptr(lengths), e.ctypes.data_as(C.c_void_p), len(e),
                                                 C.byref(p), H.ptr(t['prob']), H.ptr(t['choice']), H.ptr(t['info']), H.ptr(t['sel']), 2), 'bind')
    bind(a, l1, sk.edges_array(), 20.0)                                            # edges and parameters are copied at bind
    fwd(x1)
    bind(b, l2, e2, 35.0)
    fwd(x2)
    check(lib.metro_plan_bind_skeleton_modes(eng._plan, None, None, 0, None, None, 0, None, None, None, None, None, 0), 'unbind')
    check(lib.metro_plan_bind_modes(eng._plan, None, None, None, 0, 0, 0), 'unbind')
    fwd(x1)
    torch.cuda.synchronize()
    for t, want, n in ((a, want1, 2), (b, want2, 1)):
        for key, w in zip(('vx', 'st', 'choice', 'prob', 'info', 'sel'), want[1:]):
            assert same(t[key][:n], w), key
            assert (t[key][n:] == -7).all(), (key, 'rows n .. max_n - 1 are not touched')
    assert torch.equal(poses, want1[0])
    eng.close()


def test_more_crops_than_bound_are_refused_before_any_launch(cuda, lib):
    spec, params, radius = make_model('S2-j17')
    eng = Engine(spec, params, 'f16', max_batch=2, device=cuda)
    x = images(spec, 2, cuda)
    dummy = torch.full((4096,), -7.0, device=cuda)
    lengths = bone_rows(spec, 1, cuda)
    edges = np.ascontiguousarray(spec.skeleton.edges_array(), np.int32)
    p = MH.skeleton_mode_params(SR.SCALE)
    poses = torch.full((2, spec.skeleton.n_out, 3), -7.0, device=cuda)
    stream = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    check(lib.metro_plan_bind_skeleton_modes(eng._plan, H.ptr(dummy), H.ptr(dummy), 2, H.ptr(lengths), edges.ctypes.data_as(C.c_void_p), len(edges),
                                             C.byref(p), H.ptr(dummy), H.ptr(dummy), H.ptr(dummy), None, 1), 'bind')
    try:
        check(lib.metro_kernel_notes(1), 'notes')
        assert lib.metro_forward(eng._plan, H.ptr(x), 2, H.ptr(poses), H.ptr(eng._ws), stream) == -1
        assert b'bound skeleton buffers' in lib.metro_last_error() and lib.metro_last_kernel_id() == b''
    finally:
        check(lib.metro_kernel_notes(0), 'notes')
        check(lib.metro_plan_bind_skeleton_modes(eng._plan, None, None, 0, None, None, 0, None, None, None, None, None, 0), 'unbind')
    torch.cuda.synchronize()
    assert (poses == -7).all() and (dummy == -7).all()
    eng.close()


def test_estimate_pose_skeleton_is_forward_skeleton_modes_and_the_metric_conversion(cuda, tmp_path):
    from metro_pose3d_amd import inference as INF, save_model
    for head in ('S16-j17', 'S16-j53'):                                            # the merged output order does not carry the root
        spec, params, radius = make_model(head)
        sk = spec.skeleton
        path = str(tmp_path / f'{head}.npz')
        save_model(path, spec, params)
        x = images(spec, 3, cuda, seed=13)
        lengths = bone_rows(spec, 3, cuda)
        modes = INF.estimate_pose_modes(x, path, 3, radius, return_uncertainty=True)
        res = INF.estimate_pose_skeleton(x, path, lengths, 3, radius, return_uncertainty=True)
        host = INF.estimate_pose_skeleton(x, path, lengths.cpu().numpy(), 3, radius)
        one = INF.estimate_pose_skeleton(x, path, lengths[0].cpu().numpy(), 3, radius)
        assert len(res) == 6 and len(host) == 5 and isinstance(res[-1], INF.SkeletonModes) and isinstance(res[-2], INF.Modes)
        assert torch.equal(res[0], modes[0]) and np.array_equal(res[1], modes[1]) and list(res[2]) == list(modes[2])
        assert torch.equal(res[3].covariance, modes[3].covariance) and torch.equal(res[3].peak, modes[3].peak)
        for a, b in zip(res[-2], modes[-1]):
            assert same(a, b)
        for a, b in zip(res[-1], host[-1]):
            assert same(a, b), 'a device tensor and its host copy give equal results'
        assert all(same(a[:1], b[:1]) for a, b in zip(one[-1], host[-1])), 'an [E] table is every row\'s'
        eng = Engine(spec, params, 'f16', max_batch=8, device=cuda)
        _, vx, st, choice, prob, info, sel = eng.forward_skeleton_modes(x, lengths, 3, radius)
        s = res[-1]
        assert torch.equal(s.choice, choice) and same(s.prob, prob) and same(s.log_evidence, info[..., 0]) and same(s.log_map, info[..., 1])
        a, b = (torch.tensor(v, dtype=torch.float64, device=cuda) for v in INF._metric_map(spec))
        mm = sel.double() * a + b
        want = (mm[:, list(sk.permutation)] - mm[:, -1:]).float()
        assert same(s.poses, want)
        # the chosen modes' positions of Modes, re-rooted at the chosen root where the output order carries it
        pick = res[-2].poses.double().gather(2, choice.long().clamp(min=0)[..., None, None].expand(-1, -1, 1, 3))[:, :, 0]
        if sk.n_head - 1 in sk.permutation:
            pick = pick - pick[:, list(sk.permutation).index(sk.n_head - 1)][:, None]
        assert (pick - s.poses.double()).abs().max() < 1e-2, 'mm, fp32 roundings of two routes'
        eng.close()
        if head == 'S16-j17':                                                      # the command line: --modes K[,R] --skeleton BONES.npy
            img, bones = str(tmp_path / 'img.npy'), str(tmp_path / 'bones.npy')
            np.save(img, x[0].cpu().numpy())
            np.save(bones, lengths[0].cpu().numpy())
            INF.main(['--model-path', path, '--image', img, '--modes', '3,1', '--skeleton', bones])
            with pytest.raises(SystemExit):
                INF.main(['--model-path', path, '--image', img, '--skeleton', bones])
    INF.clear_cache()


# ---- 4: the frames layer -----------------------------------------------------------------------------------------------------------

def _frame_poses_equal(a, b):
    from tests.test_gpu_single_view import _same
    return _same(a.poses, b.poses) and _same(a.keypoints2d, b.keypoints2d) and _same(a.z_offset, b.z_offset)


def test_locate_skeleton_poses_in_frames_is_the_chain_composed_by_hand(cuda, tmp_path):
    """`plain` is locate_poses_in_frames bit for bit; `selected` is _place_poses and _merge_views on the coords01_sel of
    Engine.forward_skeleton_modes, whose rows are written out here in NumPy (repeated per view, a flipped view reading the
    mirror columns of an asymmetric table); a CUDA [n, E] tensor and its host copy give equal results."""
    from metro_pose3d_amd import frames as FR, inference as INF
    from tests.test_gpu_placement import _toy_engine_model
    from tests.test_gpu_world_follow import _rig
    spec, _, path = _toy_engine_model(tmp_path)
    sk = spec.skeleton
    cams, frames, boxes, fi, _ = _rig()
    n, e = len(boxes), len(sk.edges)
    host = np.random.default_rng(4).uniform(150.0, 450.0, (n, e))                  # asymmetric: left and right bones differ
    device = torch.from_numpy(host).to(cuda)
    em = np.asarray(sk.edge_mirror())
    assert (em >= 0).any() and (host[:, em[em >= 0]] != host[:, em >= 0]).any()
    for views in (None, 3):
        kw = dict(frame_index=fi, precision='f16', views=views, coords='world')
        want = FR.locate_poses_in_frames(frames, boxes, path, cams, bone_lengths=host, **kw)
        got = FR.locate_skeleton_poses_in_frames(frames, boxes, path, cams, host, **kw)
        on_device = FR.locate_skeleton_poses_in_frames(frames, boxes, path, cams, device, **kw)
        assert _frame_poses_equal(got.plain, want), views
        nv = 1 if views is None else views
        assert got.choice.shape == (n, nv, sk.n_out) and got.prob.shape == (n, nv, sk.n_out, 2) and got.log_evidence.shape == (n, nv, sk.n_out)
        for a, b in zip(got[2:], on_device[2:]):
            assert same(a, b)
        assert _frame_poses_equal(got.plain, on_device.plain) and _frame_poses_equal(got.selected, on_device.selected)
        # by hand
        call = FR._checked_call(frames, boxes, fi, 'world', views, 'auto', 'f16', None, 'rgb', 'bt601', 'float32')
        with torch.cuda.device(cuda):
            eng = INF._engine_for(path, 'f16', cuda, n * nv)
            crops, places = FR._warp_views(call.frames, cams, call.boxes, call.fi, call.vs, spec.proc_side, cuda, call.crop_dtype)
            rows = np.repeat(host, nv, axis=0)
            for v in np.flatnonzero(call.vs.flip):
                rows[v::nv] = host[:, np.where(em >= 0, em, np.arange(e))]
            assert views is None or call.vs.flip.any()
            d_rows = torch.from_numpy(np.ascontiguousarray(rows)).to(cuda)
            assert torch.equal(FR._view_bone_rows(device, call.vs, sk), d_rows)
            _, _, _, choice, prob, info, sel = eng.forward_skeleton_modes(crops, d_rows, 2, 1)
            targets = device if nv == 1 else device.repeat_interleave(nv, dim=0)
            poses_v, kp_v, z_v, mirror = FR._place_poses(eng, sel, None, places, 'bone-lengths', 'world', targets, 1, None)
            poses, kp, z, _ = FR._merge_views(poses_v, kp_v, z_v, places, mirror, n, nv, spread=False)
        from tests.test_gpu_single_view import _same
        assert _same(got.selected.poses, poses) and _same(got.selected.keypoints2d, kp) and _same(got.selected.z_offset, z), views
        assert torch.equal(got.choice.reshape(-1, sk.n_out), choice) and same(got.prob.reshape(-1, sk.n_out, 2), prob)
        assert same(got.log_evidence.reshape(-1, sk.n_out), info[..., 0].contiguous()) and same(got.log_map.reshape(-1, sk.n_out), info[..., 1].contiguous())
    assert torch.equal(device, torch.from_numpy(host).to(cuda)), 'the tensor is read, never written'
    # 'metro' mode: NaN says that a bone is unknown; the selected poses are skeleton_to_metric's, placed
    holes = host.copy()
    holes[:, ::3] = np.nan
    got = FR.locate_skeleton_poses_in_frames(frames, boxes, path, cams, holes, fi, scale_recovery='metro', precision='f16', coords='crop')
    want = FR.locate_poses_in_frames(frames, boxes, path, cams, fi, scale_recovery='metro', precision='f16', coords='crop')
    assert _frame_poses_equal(got.plain, want) and got.selected.z_offset is None and torch.isfinite(got.selected.poses).all()
    with pytest.raises(ValueError, match='finite and positive'):
        FR.locate_skeleton_poses_in_frames(frames, boxes, path, cams, holes, fi, precision='f16')
    for bad in (device[:, :-1], device.to(torch.float32), device[:-1]):
        with pytest.raises(ValueError, match='bone_lengths must be'):
            FR.locate_skeleton_poses_in_frames(frames, boxes, path, cams, bad, fi, precision='f16')
    INF.clear_cache()


def test_follower_locate_skeleton_is_the_call_on_its_own_bone_lengths(cuda, tmp_path):
    from metro_pose3d_amd import frames as FR, inference as INF
    from tests.test_gpu_bone_lengths import COV_SCALE
    from tests.test_gpu_placement import _toy_engine_model
    from tests.test_gpu_world_follow import _rig
    spec, _, path = _toy_engine_model(tmp_path)
    sk = spec.skeleton
    cams, frames, boxes, fi, _ = _rig()
    kw = dict(match_max_cost_mm=600.0, max_cost_mm=590.0, precision='f16', capacity=8, cov_scale=COV_SCALE)
    learn = FR.Follower(path, cams[:3], world=True, single_view='rays', learn_bones=True, **kw)
    for k in range(3):
        sel = fi // 3 == 0
        learn.follow(frames[:3], boxes[sel], fi[sel], [0.125 * k] * 3)
    fallback = np.linspace(200.0, 400.0, len(sk.edges))
    predicted = learn.predict(FR.frame_sizes(frames[:3]), [0.5] * 3)
    assert predicted.n_predicted > 0
    opts = dict(precision='f16', coords='world', k=2, radius=1)
    got = learn.locate_skeleton(frames[:3], predicted.boxes, predicted.track_index, predicted.frame_index, fallback, **opts)
    lengths = learn.bone_lengths_for(predicted.track_index, fallback)
    want = FR.locate_skeleton_poses_in_frames(frames[:3], predicted.boxes, path, cams[:3], lengths, predicted.frame_index, **opts)
    assert _frame_poses_equal(got.plain, want.plain) and _frame_poses_equal(got.selected, want.selected)
    for a, b in zip(got[2:], want[2:]):
        assert same(a, b)
    with pytest.raises(TypeError, match='bone_lengths'):
        learn.locate_skeleton(frames[:3], predicted.boxes, predicted.track_index, predicted.frame_index, fallback, bone_lengths=lengths)
    plain = FR.Follower(path, cams[:3], world=True, single_view='rays', **kw)
    plain.follow(frames[:3], boxes[fi // 3 == 0], fi[fi // 3 == 0], [0.0] * 3)
    with pytest.raises(ValueError, match='learn_bones'):
        plain.locate_skeleton(frames[:3], predicted.boxes, predicted.track_index, predicted.frame_index, fallback)
    INF.clear_cache()
