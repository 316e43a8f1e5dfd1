"""Track-predicted heat-map priors on the MI355X: toy-width synthetic models through Engine.forward_track_posterior and the frames
chain.  The rows the new kernel writes are held to the fp64 restatement (tests/track_prior_ref.py) at the bounds of
tests/test_track_prior.py (reason words equal, mu within 2.4e-7 max(1, |mu|), each precision block within 1e-6 of its largest
entry; the cases keep every decision 1e-3 s from max_age_s and 1e-1 mm from near_mm, condition number of Sigma <= 1e4); the
posterior behind them is held, bit for bit, to heads.posterior_from_logits on the same forward's dumped logits with the rows the
kernel wrote AND to Engine.forward_posterior given those rows, which together pin the order of the chain.

Heads: S = 2 (a plain logits conv) and S = 16 (the one-launch head on f16), 17 / 19 / the merged skeleton's joints, 1, 2, 64 and
65 crops, all four precisions, uint8 crops.  A plan takes depth >= 2 with depth * J_head a multiple of 4, so D is 4 and 8 here: a
volume of depth 1 cannot be bound to a forward."""
import ctypes as C

import numpy as np
import pytest
import torch

from metro_pose3d_amd import ModelSpec, _lib, frames as FR, heads as MH, synth
from metro_pose3d_amd._lib import check
from metro_pose3d_amd.engine import Engine
from tests import helpers as H, heat_posterior_ref as PR, track_prior_ref as TP
from tests.test_heat_posterior import POST_IDS

pytestmark = pytest.mark.gpu

PRECISIONS = ('f16', 'f32', 'f32m', 'f64')
PRECISE = {'f16': 0, 'f32': 1, 'f32m': 1, 'f64': 2}
# id -> (stride, proc_side, dataset, depth, crops per call, track slots, coords, depth mode, views)
HEADS = {
    'S2-D8-j17': (32, 64, 'h36m', 8, (1, 65), 128, 'world', 'root', 1),
    'S2-D4-merged': (32, 64, 'merged', 4, (64,), 1, 'camera', 'none', 1),
    'S16-D8-j19': (16, 256, 'many19', 8, (2,), 3, 'camera', 'root', 1),
    'S16-D4-j17': (16, 256, 'h36m', 4, (3,), 2, 'world', 'none', 3),
}
PLAIN = ('out', 'coords01', 'cov01', 'peak')
PARAMS = dict(TP.DEFAULTS)


def make_model(head, seed=1):
    stride, side, dataset, depth = HEADS[head][:4]
    spec = ModelSpec(50, stride, dataset, depth=depth, proc_side=side, base_width=16)
    params = synth.make_params(50, spec.n_head_channels, 16, seed=seed, logit_gain=synth.logit_gain_for(50, stride, 16))
    return spec, params


def same(a, b):
    """Bit equality of two tensors (NaN rows included)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def buffers(eng, n, cuda, heat=False):
    sk = eng.spec.skeleton
    f32 = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=cuda)
    b = dict(out=f32(n, sk.n_out, 3), coords01=f32(n, sk.n_head, 3), cov01=f32(n, sk.n_head, 6), peak=f32(n, sk.n_head))
    if heat:
        xy_shape, z_shape = eng.heat_shapes(n)
        b.update(heat_xy=f32(*xy_shape), heat_z=f32(*z_shape))
    return b


def upload(case, cuda):
    """The device tensors Engine.forward_track_posterior takes, from a restatement case."""
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    return dict(state=up(np.asarray(case['state'], np.float64)), slot=up(np.asarray(case['slot'], np.int32)),
                times=up(np.asarray(case['times'], np.float64)),
                records=up(np.ascontiguousarray(case['records']).view(np.uint8).reshape(len(case['slot']), -1)),
                mirror=up(np.asarray(case['head'].mirror, np.int32)))


def run_bound(eng, x, case, cuda, **more):
    """-> (the bound call's tensors with post, prior and reason; the unbound call's; the same forward's dumped logits)."""
    n = x.shape[0]
    b = buffers(eng, n, cuda, **more)
    t = upload(case, cuda)
    _, b['post'], b['prior'], b['reason'] = eng.forward_track_posterior(x, coords=case['coords'], depth=case['depth'], **t, **PARAMS, **b)
    u = buffers(eng, n, cuda, **more)
    step = eng.heat_chunk or n
    dumps = []
    for i in range(0, n, step):
        eng.forward(x[i:i + step], **{key: u[key][i:i + step] for key in u})
        dumps.append(eng.forward_upto(x[i:i + step], len(eng.layer_infos()) - 2))
    return b, u, torch.cat(dumps)


def hold(eng, x, case, b, u, logits, precision, what):
    """The written rows against the restatement; the posterior against the entry on the dumped logits and against the prior bind;
    every plain output against the unbound call."""
    spec = eng.spec
    ref_prior, ref_reason, margins = TP.prior(dict(case, coords01=u['coords01'].cpu().numpy()))
    TP.check_margins(margins, what)
    dev = TP.check(b['prior'].cpu().numpy(), b['reason'].cpu().numpy(), ref_prior, ref_reason, what)
    for key in u:
        assert same(b[key], u[key]), (what, key)
    step = eng.heat_chunk or x.shape[0]
    entry = torch.cat([MH.posterior_from_logits(logits[i:i + step], b['prior'][i:i + step], spec, PRECISE[precision])
                       for i in range(0, x.shape[0], step)])
    assert same(b['post'], entry), (what, 'heads.posterior_from_logits on the dumped logits and the written rows')
    assert same(b['post'], eng.forward_posterior(x, b['prior'])[1]), (what, 'Engine.forward_posterior given the written rows')
    none = b['reason'] != 0
    assert (b['post'][..., 0][none] == 0.0).all(), (what, 'no prior: log_evidence exactly 0')
    assert (b['post'][..., 0][~none] < 0.0).all() and torch.isfinite(b['post'][~none]).all(), what
    return dev


def case_for(head, spec, n, seed=3):
    _, _, _, _, _, n_tracks, coords, depth, views = HEADS[head]
    return TP.random_case(TP.Head(spec), n * views, n_tracks, coords, depth, views, seed=seed)


def gpu_deviations(cuda):
    """{key: {'mu': .., 'block': ..}} of every comparison with the restatement: what tools/track_prior_parity.py records."""
    out = {}
    for precision in PRECISIONS:
        for head in HEADS:
            spec, params = make_model(head)
            ns, views = HEADS[head][4], HEADS[head][8]
            eng = Engine(spec, params, precision, max_batch=max(ns) * views, device=cuda)
            worst = dict(mu=0.0, block=0.0)
            for n in ns:
                x = torch.from_numpy(synth.make_images(n * views, spec.proc_side, seed=7)).to(cuda)
                case = case_for(head, spec, n)
                b, u, logits = run_bound(eng, x, case, cuda)
                dev = hold(eng, x, case, b, u, logits, precision, f'{precision}/{head} n{n}')
                worst = {m: max(worst[m], dev[m]) for m in worst}
            eng.close()
            out[f'gpu/{precision}/{head}'] = worst
    return out


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('head', list(HEADS))
def test_bound_forward_against_the_restatement_and_the_chain(cuda, lib, head, precision):
    spec, params = make_model(head)
    ns, views = HEADS[head][4], HEADS[head][8]
    eng = Engine(spec, params, precision, max_batch=max(ns) * views, device=cuda)
    for n in ns:
        x = torch.from_numpy(synth.make_images(n * views, spec.proc_side, seed=7)).to(cuda)
        case = case_for(head, spec, n)
        for chunk in ((None, 32) if n > 32 else (None,)):          # 65 crops: one bound forward, and 32 + 32 + 1
            eng.heat_chunk = chunk
            b, u, logits = run_bound(eng, x, case, cuda)
            hold(eng, x, case, b, u, logits, precision, f'{precision}/{head} n{n} chunk {chunk}')
            if chunk is not None:
                assert eng.status_words(n * views).shape == (n * views,) and not eng.status_words(n * views).any()
        assert (b['reason'] == 0).any() and (n < 64 or (b['reason'] != 0).any())
    eng.heat_chunk = None
    # what the forward enqueues: unbound, the plan's own list; bound, the two launches behind it; unbound again, the plan's
    m = ns[-1] * views
    plan_ids = ' & '.join(eng.layer_kernels(m))
    t = upload(case, cuda)
    ids, unbound = [], []
    for bound in (False, True, False):
        check(lib.metro_kernel_notes(1), 'notes')
        try:
            if bound:
                eng.forward_track_posterior(x, coords=case['coords'], depth=case['depth'], **t, **PARAMS)
            else:
                unbound.append(eng.forward(x).clone())
            ids.append(lib.metro_last_kernel_id().decode())
        finally:
            check(lib.metro_kernel_notes(0), 'notes')
    assert ids[0] == plan_ids and ids[2] == plan_ids, ids
    assert ids[1] == ' & '.join((plan_ids, 'track_priors', POST_IDS[precision])), ids[1]
    assert same(unbound[0], unbound[1]), 'after unbinding, a forward gives what it gave before'
    eng.close()


@pytest.mark.parametrize('precision', ('f16', 'f32m'))
def test_uint8_crops(cuda, precision):
    """f16 reads the bytes in its first kernel (metro_forward_u8), the parity precisions expand them first: both bound."""
    head = 'S16-D8-j19'
    spec, params = make_model(head)
    eng = Engine(spec, params, precision, max_batch=2, device=cuda)
    x = torch.from_numpy(np.round(synth.make_images(2, spec.proc_side, seed=8) * 255).astype(np.uint8)).to(cuda)
    case = case_for(head, spec, 2)
    b, u, _ = run_bound(eng, x, case, cuda)
    logits = eng.forward_upto(x, len(eng.layer_infos()) - 2)
    hold(eng, x, case, b, u, logits, precision, f'{precision} uint8')
    eng.close()


@pytest.mark.parametrize('precision', ('f16', 'f64'))
def test_heat_maps_and_modes_bound_too(cuda, lib, precision):
    """With heat-maps and modes also bound, every output equals what it is when bound alone, and the launches are the marginals',
    the modes', track_priors and the posterior's, in that order, behind the plan's."""
    from tests.test_gpu_heat_marginals import HEAT_IDS
    from tests.test_gpu_heat_modes import MODES_IDS
    head = 'S16-D8-j19'
    spec, params = make_model(head)
    n = 2
    eng = Engine(spec, params, precision, max_batch=n, device=cuda)
    x = torch.from_numpy(synth.make_images(n, spec.proc_side, seed=7)).to(cuda)
    case = case_for(head, spec, n)
    t = upload(case, cuda)
    alone, _, _ = run_bound(eng, x, case, cuda)
    modes = buffers(eng, n, cuda)
    _, modes['voxel'], modes['stats'] = eng.forward_modes(x, 2, 1, **modes)
    heat = buffers(eng, n, cuda, heat=True)
    eng.forward(x, **heat)
    nj = spec.skeleton.n_out
    both = buffers(eng, n, cuda, heat=True)
    prior = torch.full((n, nj, 9), -7.0, device=cuda)
    reason = torch.full((n, nj), -7, dtype=torch.int32, device=cuda)
    post = torch.full((n, nj, 11), -7.0, device=cuda)
    scratch = torch.empty(lib.metro_plan_prior_scratch_bytes(eng._plan, n), dtype=torch.uint8, device=cuda)
    p = MH.track_prior_params(case['coords'], case['depth'], **PARAMS)
    check(lib.metro_plan_bind_track_prior(eng._plan, H.ptr(t['state']), t['state'].shape[0], H.ptr(t['slot']), H.ptr(t['times']),
                                          H.ptr(t['records']), H.ptr(t['mirror']), C.byref(p), H.ptr(prior), H.ptr(reason), H.ptr(post),
                                          H.ptr(scratch), n), 'bind')
    try:
        check(lib.metro_kernel_notes(1), 'notes')
        _, both['voxel'], both['stats'] = eng.forward_modes(x, 2, 1, **both)
        ids = lib.metro_last_kernel_id().decode()
    finally:
        check(lib.metro_kernel_notes(0), 'notes')
        check(lib.metro_plan_bind_track_prior(eng._plan, None, 0, None, None, None, None, None, None, None, None, None, 0), 'unbind')
    assert ids.endswith(' & '.join(('', HEAT_IDS[precision], MODES_IDS[precision], 'track_priors', POST_IDS[precision]))), ids[-300:]
    assert same(post, alone['post']) and same(prior, alone['prior']) and same(reason, alone['reason'])
    assert torch.equal(both['voxel'], modes['voxel']) and same(both['stats'], modes['stats'])
    for key in PLAIN + ('heat_xy', 'heat_z'):
        assert same(both[key], heat[key]), key
    eng.close()


def test_refusals_launch_nothing_and_rows_past_n_stay(cuda, lib):
    head = 'S16-D8-j19'
    spec, params = make_model(head)
    eng = Engine(spec, params, 'f16', max_batch=3, device=cuda)
    nj = spec.skeleton.n_out
    x = torch.from_numpy(synth.make_images(3, spec.proc_side, seed=9)).to(cuda)
    case = case_for(head, spec, 3)
    t = upload(case, cuda)
    prior = torch.full((3, nj, 9), -7.0, device=cuda)
    reason = torch.full((3, nj), -7, dtype=torch.int32, device=cuda)
    post = torch.full((3, nj, 11), -7.0, device=cuda)
    poses = torch.full((3, nj, 3), -7.0, device=cuda)
    c01 = torch.full((3, spec.skeleton.n_head, 3), -7.0, device=cuda)
    scratch = torch.empty(lib.metro_plan_prior_scratch_bytes(eng._plan, 2), dtype=torch.uint8, device=cuda)
    p = MH.track_prior_params(case['coords'], 'root', **PARAMS)
    stream = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    bind = lambda max_n: lib.metro_plan_bind_track_prior(eng._plan, H.ptr(t['state']), t['state'].shape[0], H.ptr(t['slot']), H.ptr(t['times']),
                                                        H.ptr(t['records']), H.ptr(t['mirror']), C.byref(p), H.ptr(prior), H.ptr(reason),
                                                        H.ptr(post), H.ptr(scratch), max_n)
    check(bind(2), 'bind')
    try:
        check(lib.metro_kernel_notes(1), 'notes')
        assert lib.metro_forward_coords01(eng._plan, H.ptr(x), 3, H.ptr(poses), H.ptr(c01), H.ptr(eng._ws), stream) == -1
        assert b'track-prior buffers' in lib.metro_last_error() and lib.metro_last_kernel_id() == b''
        assert lib.metro_forward(eng._plan, H.ptr(x), 2, H.ptr(poses), H.ptr(eng._ws), stream) == -1
        assert b'coords01' in lib.metro_last_error() and lib.metro_last_kernel_id() == b''
        assert lib.metro_plan_bind_prior(eng._plan, H.ptr(prior), H.ptr(post), H.ptr(scratch), 2) == -1
        check(lib.metro_kernel_notes(0), 'notes')
        torch.cuda.synchronize()
        assert (poses == -7).all() and (post == -7).all() and (prior == -7).all() and (reason == -7).all()
        # one crop of the two bound: rows 1 and 2 are not touched
        check(lib.metro_forward_coords01(eng._plan, H.ptr(x), 1, H.ptr(poses), H.ptr(c01), H.ptr(eng._ws), stream), 'forward')
        torch.cuda.synchronize()
        assert (post[1:] == -7).all() and (prior[1:] == -7).all() and (reason[1:] == -7).all() and (post[0] != -7).any()
    finally:
        check(lib.metro_kernel_notes(0), 'notes')
        check(lib.metro_plan_bind_track_prior(eng._plan, None, 0, None, None, None, None, None, None, None, None, None, 0), 'unbind')
    with pytest.raises(ValueError):
        eng.forward_track_posterior(x, coords='crop', **t)
    with pytest.raises(ValueError):
        eng.forward_track_posterior(x, coords='camera', **dict(t, slot=t['slot'].long()))
    with pytest.raises(ValueError):
        eng.forward_track_posterior(x, coords='camera', **dict(t, records=t['records'][:2]))
    eng.close()


def test_forward_coords01_with_the_track_prior_bound_keeps_to_a_side_stream(cuda, lib):
    """The protocol of tests/stream_harness.py on metro_forward_coords01 with the track prior bound (a chain: the bound buffers are
    no arguments of the entry): on a non-blocking side stream, behind the delay, the call returns while the delay runs, and
    poses, coords01, prior, reason and post have the bits of the default-stream run."""
    from tests import stream_harness as SH
    head = 'S16-D8-j19'
    spec, params = make_model(head)
    eng = Engine(spec, params, 'f16', max_batch=2, device=cuda)
    nj = spec.skeleton.n_out
    case = case_for(head, spec, 2)
    t = upload(case, cuda)
    p = MH.track_prior_params(case['coords'], case['depth'], **PARAMS)
    scratch = torch.empty(lib.metro_plan_prior_scratch_bytes(eng._plan, 2), dtype=torch.uint8, device=cuda)

    def fn(images):
        f32 = lambda *s: torch.full(s, -7.0, dtype=torch.float32, device=cuda)
        post, prior, poses, c01 = f32(2, nj, 11), f32(2, nj, 9), f32(2, nj, 3), f32(2, spec.skeleton.n_head, 3)
        reason = torch.full((2, nj), -7, dtype=torch.int32, device=cuda)
        check(lib.metro_plan_bind_track_prior(eng._plan, H.ptr(t['state']), t['state'].shape[0], H.ptr(t['slot']), H.ptr(t['times']),
                                              H.ptr(t['records']), H.ptr(t['mirror']), C.byref(p), H.ptr(prior), H.ptr(reason), H.ptr(post),
                                              H.ptr(scratch), 2), 'bind')
        try:
            check(lib.metro_forward_coords01(eng._plan, H.ptr(images), 2, H.ptr(poses), H.ptr(c01), H.ptr(eng._ws),
                                             C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)), 'metro_forward_coords01')
        finally:
            check(lib.metro_plan_bind_track_prior(eng._plan, None, 0, None, None, None, None, None, None, None, None, None, 0), 'unbind')
        return poses, c01, prior, reason, post
    a, b = (torch.from_numpy(synth.make_images(2, spec.proc_side, seed=s)).to(cuda) for s in (11, 12))
    SH.verdict(SH.Chain(fn, [a], [b]), cuda, what='metro_forward_coords01, track prior bound', asynchronous=True, busy=False).require_ok()
    eng.close()


# ---- the frames chain --------------------------------------------------------------------------------------------------------------

def _plain_fields(a, b):
    for name in ('poses', 'keypoints2d', 'z_offset'):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None) and (x is None or same(x, y)), name


@pytest.mark.parametrize('views', [None, 3])
@pytest.mark.parametrize('precision', ['f64', 'f16'])
def test_follow_predict_locate(cuda, tmp_path, precision, views):
    """One camera: Follower.follow on two frames, .predict for a third, .locate on the returned CUDA tensors.  `plain` is
    locate_poses_in_frames on those boxes, bit for bit; with every track_index -1 the log-evidence is exactly 0 and the posterior
    poses meet the plain ones (the posterior under no prior is the plain distribution, summed by another kernel: four times the
    coords01 deviation profiles/heat_posterior_parity.json records for the precision, seen through the back-projection).  A
    synthetic model's poses mean nothing: this checks plumbing and equivalence."""
    from metro_pose3d_amd.camera import Camera
    from tests.test_gpu_placement import _toy_engine_model
    spec, _, path = _toy_engine_model(tmp_path)
    sk = spec.skeleton
    rng = np.random.default_rng(7)
    frames = [rng.integers(0, 256, (240, 320, 3), dtype=np.uint8) for _ in range(3)]
    cam = Camera(np.array([[300.0, 0, 160], [0, 300.0, 120], [0, 0, 1]]))
    base = np.array([[20.0, 40, 70, 150], [120, 50, 80, 140], [220, 45, 75, 150]])
    boxes = np.concatenate([base, base[[2, 0, 1]] + 2.0])
    fi, stamps = np.repeat([0, 1], 3), np.arange(3) / 32.0
    follower = FR.Follower(path, cam, capacity=8, scale_recovery='true-root-depth', root_depth=3000.0 + 1000.0 * np.array([0, 1, 2, 2, 0, 1]),
                           precision=precision, views=views)
    follower.follow(frames[:2], boxes, fi, stamps[:2])
    kept = [t.clone() for t in follower.tracks]
    pred = follower.predict(FR.frame_sizes(frames[2:]), stamps[2:], max_sigma_mm=100.0)
    n = len(pred.boxes)
    assert n >= 1 and pred.boxes.is_cuda and pred.track_index.is_cuda
    root = 3000.0 + 1000.0 * np.arange(n)
    got = follower.locate(frames[2:], pred.boxes, pred.track_index, pred.frame_index, stamps[2:], root_depth=root)
    assert all(same(a, b) for a, b in zip(follower.tracks, kept)), 'the table is read, never written'
    plain = FR.locate_poses_in_frames(frames[2:], pred.boxes, path, cam, pred.frame_index, scale_recovery='true-root-depth', root_depth=root,
                                      precision=precision, views=views)
    _plain_fields(got.plain, plain)
    nv = 1 if views is None else views
    assert got.log_evidence.shape == got.peak.shape == got.reason.shape == (n, nv, sk.n_out) and got.reason.dtype == torch.int32
    assert got.posterior.poses.shape == plain.poses.shape and got.posterior_covariance.shape == (n, sk.n_out, 3, 3)
    assert ((got.log_evidence == 0) == (got.reason != 0)).all() and (got.log_evidence <= 0).all()
    print(f'{precision} views {views}: {n} boxes, reasons {torch.bincount(got.reason.reshape(-1), minlength=7).tolist()}, '
          f'log-evidence min {float(got.log_evidence.min()):.3f}')
    assert (got.reason == 0).any(), 'a followed person has a prior'
    # no track at all: the plain distribution through the posterior kernel
    free = follower.locate(frames[2:], pred.boxes, torch.full_like(pred.track_index, -1), pred.frame_index, stamps[2:], root_depth=root)
    _plain_fields(free.plain, plain)
    assert (free.reason == 1).all() and (free.log_evidence == 0).all()
    rec = PR.recorded()['worst']
    grid = 4.0 * max(v['grid'] for key, v in rec.items() if key.startswith(f'gpu/{precision}/'))
    # a deviation of `grid` voxel steps of the S = 8, D = 8 volume in mm: a step is lrc / 7 crop pixels across and box / 7 mm along
    # z; a crop pixel is depth / f_virtual mm, below twice box / proc_side here (roots at most 5 m away, boxes of 140 px and more
    # under f = 300); three axes, and as much again for the root's own deviation, which moves every joint
    last = spec.proc_side - 1
    lrc = last - last % spec.stride - 1
    bound_mm = 2.0 * grid * max(lrc / 7.0 * spec.box_size_mm / spec.proc_side, spec.box_size_mm / 7.0) * np.sqrt(3.0) * 2.0
    worst = float((free.posterior.poses - plain.poses).abs().max())
    print(f'{precision} views {views}: posterior under no prior vs plain: {worst:.3e} mm (bound {bound_mm:.3e} mm)')
    assert worst <= bound_mm
    host = follower.locate(frames[2:], pred.boxes.cpu().numpy(), pred.track_index.cpu().numpy(), pred.frame_index.cpu().numpy(), stamps[2:],
                           root_depth=root, geometry='device')
    assert same(host.log_evidence, got.log_evidence) and same(host.posterior.poses, got.posterior.poses) and same(host.reason, got.reason)
    from metro_pose3d_amd import inference as INF
    INF.clear_cache()


def test_rig_table_in_the_world_with_depth_root(cuda, tmp_path):
    """A table in the world seen by a 3-camera rig, depth='root': locate_tracked_poses_in_frames(table_coords='world') gives reason 0
    for the tracked rows, and its reason words and log-evidence are those of Engine.forward_track_posterior on the chain's own
    crops and records, whose prior rows meet the restatement."""
    from metro_pose3d_amd.inference import _engine_for, clear_cache
    from tests import triangulation_ref as TR
    from tests.test_gpu_placement import _toy_engine_model
    spec, _, path = _toy_engine_model(tmp_path)
    sk = spec.skeleton
    head = TP.Head(spec)
    rng = np.random.default_rng(5)
    cams = TR.ring_cameras([0, 100, 215], focal=260.0, principal=(160.0, 120.0))
    frames = [rng.integers(0, 256, (240, 320, 3), dtype=np.uint8) for _ in cams]
    # two persons near the ring's centre, 4.5 m from every camera; slot 1 and slot 3 of a table of 4
    state = TP.empty_state(4, sk.n_out)
    for s, centre in ((1, (200.0, -300.0, 1000.0)), (3, (600.0, 100.0, 1100.0))):
        for r in range(sk.n_out):
            x = np.concatenate([np.asarray(centre) + rng.uniform(-350, 350, 3), rng.uniform(-500, 500, 3)])
            state[s, r] = TP.pack_state(x, TP.random_cov6(rng), 1.0)
    table = FR.TrackTable(torch.from_numpy(state).to(cuda), torch.tensor([-1, 0, -1, 1], dtype=torch.int32, device=cuda),
                          torch.tensor([2], dtype=torch.int32, device=cuda))
    boxes = np.array([[100.0, 40, 90, 160], [150, 50, 80, 150], [110, 45, 85, 155], [160, 40, 80, 160], [120, 50, 80, 150], [90, 40, 90, 160],
                      [10.0, 10, 60, 100]])
    fi = np.array([0, 0, 1, 1, 2, 2, 0])
    slots = np.array([1, 3, 1, 3, 1, 3, -1])
    stamps = [1.04, 1.04, 1.04]
    root = np.full(len(boxes), 4500.0)
    kw = dict(scale_recovery='true-root-depth', root_depth=root, precision='f64', coords='world')
    got = FR.locate_tracked_poses_in_frames(frames, boxes, path, cams, table, slots, fi, stamps, table_coords='world', depth='root', **kw)
    plain = FR.locate_poses_in_frames(frames, boxes, path, cams, fi, **kw)
    _plain_fields(got.plain, plain)
    reason = got.reason[:, 0]
    print(f'rig: reasons {torch.bincount(reason.reshape(-1), minlength=7).tolist()}')
    assert (reason[:6] == 0).all() and (reason[6] == 1).all() and (got.log_evidence[:6] < 0).all() and (got.log_evidence[6] == 0).all()
    # the chain's own pieces, by hand
    call = FR._checked_call(frames, boxes, fi, 'world', None, 'auto', 'f64', None, 'rgb', 'bt601')
    with torch.cuda.device(cuda):
        eng = _engine_for(path, 'f64', cuda, len(boxes))
        crops, places = FR._warp_views(call.frames, cams, call.boxes, call.fi, call.vs, spec.proc_side, cuda)
        c01 = torch.empty((len(boxes), sk.n_head, 3), device=cuda)
        times = torch.tensor([1.04] * len(boxes), dtype=torch.float64, device=cuda)
        _, post, prior, why = eng.forward_track_posterior(crops, table.state, torch.from_numpy(slots.astype(np.int32)).to(cuda), times, places,
                                                          torch.tensor(sk.out_mirror, dtype=torch.int32, device=cuda), 'world', 'root',
                                                          coords01=c01)
    assert same(why, got.reason[:, 0]) and same(post[..., 0].contiguous(), got.log_evidence[:, 0].contiguous())
    case = dict(head=head, state=state, slot=slots, times=np.full(len(boxes), 1.04), coords='world', depth='root', params=dict(TP.DEFAULTS),
                records=np.frombuffer(places.cpu().numpy().tobytes(), TP.PLACEMENT), coords01=c01.cpu().numpy())
    ref_prior, ref_reason, margins = TP.prior(case)
    TP.check_margins(margins, 'rig')
    TP.check(prior.cpu().numpy(), why.cpu().numpy(), ref_prior, ref_reason, 'rig, world table, depth root')
    root_row = head.root_out
    assert (prior[:6, :, 5] > 0)[:, [r for r in range(sk.n_out) if r != root_row]].all() and (prior[:6, root_row, 5] == 0).all()
    clear_cache()
