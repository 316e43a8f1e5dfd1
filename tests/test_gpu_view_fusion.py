"""The view fusion on the MI355X: toy-width synthetic models, the forward as the vehicle of the bound launch.  What the kernel
writes is held to the fp64 restatement (tests/view_fusion_ref.py) at the bounds of tests/test_view_fusion.py -- integers exact,
points within 1e-3 mm, each covariance block within 1e-6 of its largest entry, peak and agreement within 4 fp32 ulps or 1e-6, after
the margins of every case have been asserted -- first on hand-filled marginals (the CPU cases; 1, 2 and 65 persons), then on the
marginals the same forward wrote.  The internal centres are heads.triangulate_joints' points bit for bit; every other output of
the forward keeps the bits of the unbound call; frames.fuse_poses_in_frames is its chain composed by hand."""
import ctypes as C

import numpy as np
import pytest
import torch

from metro_pose3d_amd import ModelSpec, _lib, frames as FR, heads as MH, synth
from metro_pose3d_amd._lib import check
from metro_pose3d_amd.engine import Engine
from tests import helpers as H, view_fusion_ref as VF

pytestmark = pytest.mark.gpu

# id -> (stride, proc_side, dataset, depth): S = 8 with 17 joints, S = 16 with 19
HEADS = {'S8-j17': (32, 256, 'h36m', 8), 'S16-j19': (16, 256, 'many19', 8)}


def make_model(head, seed=1):
    stride, side, dataset, depth = HEADS[head]
    spec = ModelSpec(50, stride, dataset, depth=depth, proc_side=side, base_width=16)
    params = synth.make_params(50, spec.n_head_channels, 16, seed=seed, logit_gain=synth.logit_gain_for(50, stride, 16))
    return spec, params


def head_of(spec):
    return VF.head_of(spec.proc_side, spec.stride, spec.centered_stride)


def same(a, b):
    """Bit equality of two tensors (NaN rows included)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def images(n, spec, cuda, seed=7, u8=False):
    x = synth.make_images(n, spec.proc_side, seed=seed)
    return torch.from_numpy(np.round(x * 255).astype(np.uint8) if u8 else x).to(cuda)


def upload(case, cuda):
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    return dict(xy=up(case['xy']), records=up(np.ascontiguousarray(case['records']).view(np.uint8).reshape(case['n'], -1)),
                rows=up(np.asarray(case['rows'], np.int32)), starts=up(np.asarray(case['starts'], np.int32)),
                mirror=up(np.asarray(case['mirror'], np.int32)), centres=up(np.asarray(case['centres'], np.float32)))


def outputs(n_persons, n_out, cuda):
    f32 = lambda k: torch.full((n_persons, n_out, k), -7.0, dtype=torch.float32, device=cuda)
    return dict(points=f32(3), cov=f32(9), stats=f32(2), info=torch.full((n_persons, n_out, 2), -7, dtype=torch.int32, device=cuda),
                centres_out=f32(3))


def bind(lib, eng, t, o, params, max_n, centres=True):
    n_persons = t['starts'].numel() - 1
    return lib.metro_plan_bind_view_fusion(eng._plan, H.ptr(t['xy']), H.ptr(t['records']), H.ptr(t['rows']), t['rows'].numel(), H.ptr(t['starts']),
                                           n_persons, H.ptr(t['mirror']), H.ptr(t['centres']) if centres else None, C.byref(params),
                                           H.ptr(o['points']), H.ptr(o['cov']), H.ptr(o['stats']), H.ptr(o['info']), H.ptr(o['centres_out']),
                                           max_n)


def unbind(lib, eng):
    check(lib.metro_plan_bind_view_fusion(eng._plan, None, None, None, 0, None, 0, None, None, None, None, None, None, None, None, 0), 'unbind')


def fusion_record(case, weights='uniform'):
    par = case['params']
    return MH.fusion_params(par['grid'], par['extent_mm'], par['floor'], par['near_mm']).record(weights, 2.0, par['n_views'])


def run_crafted(lib, eng, case, cuda, x):
    """The forward with the fusion bound to the case's hand-filled tensors -> the four outputs on the host, and centres_out."""
    t = upload(case, cuda)
    o = outputs(len(case['starts']) - 1, len(case['mirror']), cuda)
    check(bind(lib, eng, t, o, fusion_record(case), case['n']), 'metro_plan_bind_view_fusion')
    try:
        eng.forward(x)
    finally:
        unbind(lib, eng)
    torch.cuda.synchronize()
    assert same(o['centres_out'], t['centres']), 'the centres are copied bit for bit'
    return tuple(o[k].cpu().numpy() for k in ('points', 'cov', 'stats', 'info'))


# ---- 1: crafted inputs --------------------------------------------------------------------------------------------------------------

PERSONS = {1: (3,), 2: (3, 2), 65: tuple(p % 3 for p in range(65))}          # 65 persons: 64 rows and a spare one, 65 crops


@pytest.mark.parametrize('n_persons', list(PERSONS))
@pytest.mark.parametrize('head', list(HEADS))
def test_crafted_inputs_against_the_restatement(cuda, lib, head, n_persons):
    """1, 2 and 65 persons (groups of 0, 1, 2 and 3 rows; 1105 workgroups at 65 x 17) on hand-filled marginals, records, CSR and
    centres, at the default grid of 16 and at grids 2 and 3."""
    spec, params = make_model(head)
    counts = PERSONS[n_persons]
    grids = (16, 2, 3) if n_persons == 2 else (16,)
    n = sum(counts) + 1
    eng = Engine(spec, params, 'f16', max_batch=n, device=cuda)
    x = images(n, spec, cuda)
    for grid in grids:
        case = VF.make_case(head_of(spec), spec.skeleton.n_out, counts, seed=60 + n_persons + grid, stride=spec.stride, grid=grid)
        ref = VF.fuse(case)
        worst = VF.check(run_crafted(lib, eng, case, cuda, x), ref)
        print(f'{head} persons {n_persons} grid {grid}: {worst} margins {ref["margins"]}')
        assert (ref['n_rows'] == np.asarray(counts)[:, None]).all()
    eng.close()


def gpu_deviations(cuda):
    """{key: worst deviations} of the crafted comparisons with the restatement: what tools/view_fusion_parity.py records."""
    lib, out = _lib.load(), {}
    for head in HEADS:
        spec, params = make_model(head)
        for n_persons, counts in PERSONS.items():
            n = sum(counts) + 1
            eng = Engine(spec, params, 'f16', max_batch=n, device=cuda)
            case = VF.make_case(head_of(spec), spec.skeleton.n_out, counts, seed=60 + n_persons + 16, stride=spec.stride)
            out[f'gpu/{head}/persons{n_persons}'] = VF.check(run_crafted(lib, eng, case, cuda, images(n, spec, cuda)), VF.fuse(case))
            eng.close()
    return out


@pytest.mark.parametrize('name', ('flipped-view', 'nan-map', 'non-finite-record', 'row-index-outside', 'behind-a-camera',
                                  'outside-the-map', 'nan-centre', 'rows-33', 'views-3'))
def test_crafted_single_cases(cuda, lib, name):
    """The single cases of the CPU tests through the launch; 33 rows in one group (two full chunks of row records and one row)
    and three rows per camera."""
    head = 'S16-j19'
    spec, params = make_model(head)
    n_out = spec.skeleton.n_out
    if name == 'rows-33':
        case = VF.make_case(head_of(spec), n_out, (33, 17, 16), seed=71, stride=spec.stride, grid=8, spare_rows=0)
    elif name == 'views-3':
        case = VF.make_case(head_of(spec), n_out, (6, 3), seed=72, stride=spec.stride, n_views=3)
    else:
        case = VF.single_cases(head_of(spec), n_out, spec.stride)[name]
        case['behind'], case['outside'] = VF.count_floor_points(case)
    eng = Engine(spec, params, 'f16', max_batch=case['n'], device=cuda)
    ref = VF.fuse(case)
    worst = VF.check(run_crafted(lib, eng, case, cuda, images(case['n'], spec, cuda)), ref)
    print(f'{name}: {worst} margins {ref["margins"]}')
    if name not in ('rows-33', 'views-3'):
        VF.check_single(name, case, ref)
    eng.close()


def test_refusals_launch_nothing_and_a_smaller_batch_skips_its_rows(cuda, lib):
    head = 'S8-j17'
    spec, params = make_model(head)
    case = VF.make_case(head_of(spec), spec.skeleton.n_out, (2, 2), seed=81, stride=spec.stride, spare_rows=0)
    eng = Engine(spec, params, 'f16', max_batch=4, device=cuda)
    x, t = images(4, spec, cuda), upload(case, cuda)
    o = outputs(2, spec.skeleton.n_out, cuda)
    poses = torch.full((4, spec.skeleton.n_out, 3), -7.0, device=cuda)
    c01 = torch.full((4, spec.skeleton.n_head, 3), -7.0, device=cuda)
    stream = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    try:
        check(bind(lib, eng, t, o, fusion_record(case, 'covariance'), 3, centres=False), 'bind')
        check(lib.metro_kernel_notes(1), 'notes')
        assert lib.metro_forward_coords01(eng._plan, H.ptr(x), 4, H.ptr(poses), H.ptr(c01), H.ptr(eng._ws), stream) == -1
        assert b'view-fusion buffers' in lib.metro_last_error() and lib.metro_last_kernel_id() == b''
        assert lib.metro_forward(eng._plan, H.ptr(x), 3, H.ptr(poses), H.ptr(eng._ws), stream) == -1
        assert b'coords01' in lib.metro_last_error() and lib.metro_last_kernel_id() == b''
        assert lib.metro_forward_coords01(eng._plan, H.ptr(x), 3, H.ptr(poses), H.ptr(c01), H.ptr(eng._ws), stream) == -1
        assert b'cov01' in lib.metro_last_error() and lib.metro_last_kernel_id() == b''
        check(lib.metro_kernel_notes(0), 'notes')
        torch.cuda.synchronize()
        assert (poses == -7).all() and all((v == -7).all() for v in o.values())
        # a forward of fewer crops than the rows name: the rows at and past n are skipped, as a row index outside [0, n)
        n = 3
        check(bind(lib, eng, t, o, fusion_record(case), 4), 'bind')
        eng.forward(x[:n])
        torch.cuda.synchronize()
        ref = VF.fuse(dict(case, n=n))
        VF.check(tuple(o[k].cpu().numpy() for k in ('points', 'cov', 'stats', 'info')), ref)
        assert ref['n_rows'].sum() == 3 * spec.skeleton.n_out
    finally:
        check(lib.metro_kernel_notes(0), 'notes')
        unbind(lib, eng)
    eng.close()


# ---- 2: the internal centres --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('u8', (False, True), ids=('fp32-crops', 'uint8-crops'))
@pytest.mark.parametrize('weights', ('uniform', 'covariance'))
@pytest.mark.parametrize('precision', ('f16', 'f64'))
def test_internal_centres_are_the_triangulation(cuda, lib, precision, weights, u8):
    """Without centres the forward triangulates its own coords01 (and cov01): centres_out is heads.triangulate_joints on the
    returned tensors bit for bit, and every fusion output has the bits of a second bound forward that is GIVEN those centres
    (the path the crafted cases hold to the restatement).  A synthetic model's rays meet nowhere in particular, so the cubes
    may stand where every row gives the floor and the largest energy leads nothing: the restatement is asked for the rows used
    only, which no margin guards."""
    head = 'S8-j17'
    spec, params = make_model(head)
    sk = spec.skeleton
    case = VF.make_case(head_of(spec), sk.n_out, (3, 2, 0, 4), seed=91, stride=spec.stride)
    n = case['n']
    eng = Engine(spec, params, precision, max_batch=n, device=cuda)
    x, t = images(n, spec, cuda, u8=u8), upload(case, cuda)
    o = outputs(4, sk.n_out, cuda)
    f32 = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=cuda)
    c01, cov01, peak = f32(n, sk.n_head, 3), f32(n, sk.n_head, 6), f32(n, sk.n_head)
    check(bind(lib, eng, t, o, fusion_record(case, weights), n, centres=False), 'bind')
    try:
        check(lib.metro_kernel_notes(1), 'notes')
        eng.forward(x, coords01=c01, cov01=cov01, peak=peak)
        ids = lib.metro_last_kernel_id().decode()
    finally:
        check(lib.metro_kernel_notes(0), 'notes')
        unbind(lib, eng)
    assert ids.endswith(' & triangulate_joints & view_fusion<g16>'), ids[-200:]
    want = MH.triangulate_joints(c01, cov01, t['records'].reshape(-1), t['rows'], t['starts'], spec, weights)[0]
    assert same(o['centres_out'], want), 'centres_out against heads.triangulate_joints'
    words = eng.status_words(n).clone()
    given = outputs(4, sk.n_out, cuda)
    t_given = dict(t, centres=o['centres_out'].clone())        # kept alive: the plan holds its address until the unbind
    check(bind(lib, eng, t_given, given, fusion_record(case, weights), n), 'bind')
    try:
        eng.forward(x, coords01=c01, cov01=cov01, peak=peak)
    finally:
        unbind(lib, eng)
    assert torch.equal(eng.status_words(n), words) and not words.any()
    for key in o:
        assert same(o[key], given[key]), (key, int((o[key].view(torch.int32) != given[key].view(torch.int32)).sum()), o[key].numel())
    # the rows used around those centres: the restatement given them
    ref = VF.fuse(dict(case, centres=o['centres_out'].cpu().numpy()))
    info = o['info'].cpu().numpy()
    assert np.array_equal(info[..., 0], ref['n_rows']) and (info[2] == 0).all()
    solved = torch.isfinite(want).all(dim=-1).cpu().numpy()
    assert np.array_equal(info[..., 0] > 0, solved & (ref['n_rows'] > 0))
    eng.close()


# ---- 3: bound to the marginals of the same forward ---------------------------------------------------------------------------------

@pytest.mark.parametrize('precision', ('f16', 'f64'))
@pytest.mark.parametrize('head', list(HEADS))
def test_bound_to_the_forwards_own_marginals(cuda, lib, head, precision):
    """Engine.forward_view_fusion: d_xy is the heat_xy the same forward writes, the fusion launch behind the marginal launches.
    The outputs meet the restatement on the returned heat_xy; every other output has the bits of the unbound call."""
    from tests.test_gpu_heat_marginals import HEAT_IDS
    spec, params = make_model(head)
    sk = spec.skeleton
    case = VF.make_case(head_of(spec), sk.n_out, (3, 2), seed=101, stride=spec.stride, grid=8)
    n = case['n']
    eng = Engine(spec, params, precision, max_batch=n, device=cuda)
    x, t = images(n, spec, cuda), upload(case, cuda)
    f32 = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=cuda)
    buffers = lambda: dict(out=f32(n, sk.n_out, 3), coords01=f32(n, sk.n_head, 3), cov01=f32(n, sk.n_head, 6), peak=f32(n, sk.n_head),
                           heat_xy=f32(*eng.heat_shapes(n)[0]), heat_z=f32(*eng.heat_shapes(n)[1]))
    b, u = buffers(), buffers()
    fusion = MH.fusion_params(grid=8)
    plan_ids = ' & '.join(eng.layer_kernels(n))
    check(lib.metro_kernel_notes(1), 'notes')
    try:
        _, _, points, cov, stats, info, centres = eng.forward_view_fusion(x, t['records'], t['rows'], t['starts'], 2, t['mirror'], fusion,
                                                                          'uniform', centres=t['centres'], **b)
        ids = lib.metro_last_kernel_id().decode()
    finally:
        check(lib.metro_kernel_notes(0), 'notes')
    # the plan's launches (the head's in their moments form: cov01 and peak are asked for), the marginals', the fusion's
    assert ids.count(' & ') == plan_ids.count(' & ') + HEAT_IDS[precision].count(' & ') + 2 and 'triangulate' not in ids
    assert ids.endswith(' & '.join(('', HEAT_IDS[precision], 'view_fusion<g8>'))), ids[-300:]
    bound_words = eng.status_words(n).clone()                   # before the next forward writes them again
    eng.forward(x, **u)
    words = eng.status_words(n).clone()
    for key in u:
        assert same(b[key], u[key]), key
    assert torch.equal(bound_words, words) and not words.any() and same(centres, t['centres'])
    ref = VF.fuse(dict(case, xy=b['heat_xy'].cpu().numpy()))
    worst = VF.check(tuple(a.cpu().numpy() for a in (points, cov, stats, info)), ref)
    print(f'{head} {precision}: {worst} margins {ref["margins"]}')
    # and with the internal centres, behind the triangulation launch: the same forward outputs, centres from the returned coords01
    got = eng.forward_view_fusion(x, t['records'], t['rows'], t['starts'], 2, t['mirror'], fusion, 'covariance')
    assert torch.equal(eng.status_words(n), words), 'the status words of the bound call with internal centres'
    assert same(got[0], u['out']) and same(got[1], u['coords01'])
    assert same(got[6], MH.triangulate_joints(u['coords01'], u['cov01'], t['records'].reshape(-1), t['rows'], t['starts'], spec, 'covariance')[0])
    with pytest.raises(ValueError, match='share one forward'):
        eng.heat_chunk = 2
        eng.forward_view_fusion(x, t['records'], t['rows'], t['starts'], 2, t['mirror'], fusion)
    eng.heat_chunk = None
    for bad in (dict(rows=t['rows'].long()), dict(starts=t['starts'][:2]), dict(records=t['records'][:2]), dict(mirror=t['mirror'][:3])):
        kw = dict(dict(records=t['records'], rows=t['rows'], starts=t['starts'], mirror=t['mirror']), **bad)
        with pytest.raises(ValueError):
            eng.forward_view_fusion(x, kw['records'], kw['rows'], kw['starts'], 2, kw['mirror'], fusion)
    eng.close()


def test_forward_view_fusion_keeps_to_a_side_stream(cuda):
    """The protocol of tests/stream_harness.py on Engine.forward_view_fusion with the internal centres (a chain of the forward,
    the marginal launches, the triangulation and the fusion): on a non-blocking side stream, behind the delay, the call returns
    while the delay runs, and every output has the bits of the default-stream run."""
    from tests import stream_harness as SH
    head = 'S8-j17'
    spec, params = make_model(head)
    case = VF.make_case(head_of(spec), spec.skeleton.n_out, (2, 2), seed=111, stride=spec.stride, spare_rows=0)
    eng = Engine(spec, params, 'f16', max_batch=4, device=cuda)
    t = upload(case, cuda)
    fusion = MH.fusion_params(grid=8)
    fn = lambda x: eng.forward_view_fusion(x, t['records'], t['rows'], t['starts'], 2, t['mirror'], fusion, 'covariance')
    a, b = (images(4, spec, cuda, seed=s) for s in (11, 12))
    SH.verdict(SH.Chain(fn, [a], [b]), cuda, what='Engine.forward_view_fusion', asynchronous=True, busy=False).require_ok()
    eng.close()


# ---- 4: the public call ---------------------------------------------------------------------------------------------------------------

def _rig_scene():
    """3 cameras on a ring with 320 x 240 frames of noise; persons 0 and 1 boxed in every frame, person 2 in frame 0 only."""
    from tests import triangulation_ref as TR
    rng = np.random.default_rng(21)
    cams = TR.ring_cameras([0, 100, 215], focal=260.0, principal=(160.0, 120.0))
    frames = [rng.integers(0, 256, (240, 320, 3), dtype=np.uint8) for _ in cams]
    boxes = np.array([[60.0, 40, 70, 150], [170, 50, 80, 140], [50, 30, 90, 160], [180, 60, 60, 120], [90, 45, 75, 150],
                      [200, 40, 70, 160], [10, 10, 60, 100]])
    return cams, frames, boxes, np.array([0, 0, 1, 1, 2, 2, 0]), np.array([0, 1, 0, 1, 0, 1, 2])


@pytest.mark.parametrize('views', [None, 3], ids=['one-view', 'three-views'])
def test_fuse_poses_in_frames_is_the_chain_composed_by_hand(cuda, tmp_path, views):
    """.world is triangulate_poses_in_frames' result bit for bit; the fused outputs are Engine.forward_view_fusion's on the chain's
    own crops and records; a side stream gives the same bits.  f32m: its forward gives a batch the same bits in every call.
    A synthetic model's poses mean nothing: this checks plumbing and equivalence."""
    from metro_pose3d_amd.inference import _engine_for, clear_cache
    from tests import stream_harness as SH
    from tests.test_gpu_placement import _toy_engine_model
    spec, _, path = _toy_engine_model(tmp_path)
    sk = spec.skeleton
    cams, frames, boxes, fi, pi = _rig_scene()
    vs = FR.view_set(1 if views is None else views)
    n, nv = len(boxes), len(vs.zoom)
    kw = dict(views=views, precision='f32m', grid=8, extent_mm=900.0)
    for weights in ('covariance', 'uniform'):
        got = FR.fuse_poses_in_frames(frames, boxes, path, cams, pi, fi, weights=weights, **kw)
        world = FR.triangulate_poses_in_frames(frames, boxes, path, cams, pi, fi, weights=weights, views=views, precision='f32m')
        for name in ('poses', 'n_rays', 'residual', 'keypoints2d'):
            assert same(getattr(got.world, name), getattr(world, name)), (weights, name)
        with torch.cuda.device(cuda):
            eng = _engine_for(path, 'f32m', cuda, n * nv)
            crops, places = FR._warp_views(frames, cams, boxes, fi, vs, spec.proc_side, cuda)
            rows, starts = (torch.from_numpy(a).to(cuda) for a in FR.person_groups(pi, fi, nv))
            mirror = torch.tensor(sk.out_mirror, dtype=torch.int32, device=cuda)
            _, _, points, cov, stats, info, centres = eng.forward_view_fusion(crops, places.reshape(n * nv, -1), rows, starts, 3, mirror,
                                                                              MH.fusion_params(8, 900.0), weights, n_views=nv)
        assert same(got.poses, points) and same(got.covariance, cov.view(3, sk.n_out, 3, 3))
        assert same(got.peak.contiguous(), stats[..., 0].contiguous()) and same(got.agreement.contiguous(), stats[..., 1].contiguous())
        assert same(got.n_rows.contiguous(), info[..., 0].contiguous()) and same(got.edge.contiguous(), info[..., 1].contiguous())
        assert same(centres, world.poses), 'the cubes stand around the triangulated joints'
        assert got.poses.shape == (3, sk.n_out, 3) and got.n_rows.dtype == torch.int32
        solved = torch.isfinite(world.poses).all(dim=-1)
        assert ((got.n_rows > 0) == solved).all() and (got.n_rows[solved] == 3 * nv).all() and torch.isnan(got.poses[2]).all()
        assert (got.agreement[solved] <= 0).all() and torch.isfinite(got.poses[solved]).all()
    side = SH.side_stream(cuda)
    with torch.cuda.stream(side):
        again = FR.fuse_poses_in_frames(frames, boxes, path, cams, pi, fi, weights='uniform', **kw)
    side.synchronize()
    for name in ('poses', 'covariance', 'peak', 'agreement', 'n_rows', 'edge'):
        assert same(getattr(again, name).contiguous(), getattr(got, name).contiguous()), name
    assert same(again.world.poses, got.world.poses)
    empty = FR.fuse_poses_in_frames(frames, np.zeros((0, 4)), path, cams, [], [], **kw)
    assert empty.poses.shape == (0, sk.n_out, 3) and empty.covariance.shape == (0, sk.n_out, 3, 3) and empty.world.poses.shape[0] == 0
    clear_cache()
