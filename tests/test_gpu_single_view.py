"""metro_person_steps_labels, metro_person_rays, metro_associate_tracks_rays and frames.follow_rig_poses_in_frames on the MI355X:
the three launches against their fp64 restatement (tests/single_view_ref.py) on the cases and bounds of tests/test_single_view.py,
the association's working state against what metro_smooth_tracks writes, and the whole call against the composition by hand of
the heads launches, whole and cut in two, and against follow_world_poses_in_frames with single_view='skip'."""
import numpy as np
import pytest
import torch

from metro_pose3d_amd import frames as FR, heads as MH
from tests import assign_tracks_ref as AR
from tests import single_view_ref as SV
from tests import triangulation_ref as TR
from tests import world_follow_ref as WR
from tests.assoc_host import NO_RAY_ROW_CASES, assert_ray_walk_is_the_plain_walk, without_ray_rows

gpu = pytest.mark.gpu
LABEL_CASES = SV.labels_cases()


def _up(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


# ---- the three launches -------------------------------------------------------------------------------------------------------------

def _labels(c, cuda):
    if len(c['person_index']) != c['n']:                   # more boxes than persons: the C entry itself
        import ctypes as C
        from metro_pose3d_amd import _lib
        dev = lambda a, dtype: _up(np.ascontiguousarray(a, dtype), cuda)
        ins = [dev(c['person_index'], np.int32), dev([c['n_persons']], np.int32), dev(c['box_step'], np.int32), dev(c['step_times'], np.float64)]
        n, n_steps = c['n'], len(c['step_times'])
        i32 = lambda k: torch.full((k,), SV.SENTINEL, dtype=torch.int32, device=cuda)
        outs = [i32(n), torch.full((n,), float(SV.SENTINEL), dtype=torch.float64, device=cuda), i32(n), i32(n_steps + 1), i32(n)]
        p = lambda t: C.c_void_p(t.data_ptr())
        with torch.cuda.device(cuda):
            _lib.check(_lib.load().metro_person_steps_labels(p(ins[0]), p(ins[1]), n, p(ins[2]), len(c['box_step']), p(ins[3]), n_steps,
                                                             *(p(t) for t in outs), C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)),
                       'metro_person_steps_labels')
        return tuple(outs)
    return MH.person_steps_labels(_up(c['person_index'], cuda), _up(np.asarray([c['n_persons']], np.int32), cuda), c['box_step'],
                                  c['step_times'])


@gpu
@pytest.mark.parametrize('name', list(LABEL_CASES))
def test_person_steps_labels_launch_matches_the_restatement(cuda, name):
    c = LABEL_CASES[name]
    got = _labels(c, cuda)
    assert [t.dtype for t in got] == [torch.int32, torch.float64, torch.int32, torch.int32, torch.int32]
    got = [t.cpu().numpy() for t in got]
    want = SV.person_steps_labels(**c)
    WR.compare_person_steps(got[:4], want[:4])
    assert np.array_equal(got[4], want[4])
    print(f"{name}: {int((got[4] >= 0).sum())} of {c['n']} persons single, {int((got[0] >= 0).sum())} with a step")


@gpu
@pytest.mark.parametrize('name', ['n2-pair', 'n127-mixed', 'n128-mixed', 'n128-pairs', 'label-out-of-range'])
def test_labels_launch_gives_metro_person_steps_values_for_persons_with_several_boxes(cuda, name):
    c = LABEL_CASES[name]
    n = c['n']
    groups = [np.flatnonzero(c['person_index'] == p) for p in range(n)]
    groups = [g if len(g) > 1 else g[:0] for g in groups]                 # metro_cluster_views: a single box has an empty group
    rows = np.concatenate(groups + [np.full(n - sum(map(len, groups)), -1)]).astype(np.int32)
    starts = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
    count = _up(np.asarray([c['n_persons']], np.int32), cuda)
    old = MH.person_steps(_up(rows, cuda), _up(starts, cuda), count, c['box_step'], c['step_times'])
    new = _labels(c, cuda)
    several = _up(np.array([len(g) > 1 for g in groups]), cuda)
    assert several.any() and torch.equal(old[0][several], new[0][several])
    assert np.array_equal(old[1][several].cpu().numpy(), new[1][several].cpu().numpy(), equal_nan=True)
    assert (old[0][~several] == -1).all()


@gpu
@pytest.mark.parametrize('name', list(SV.RAY_CASES))
def test_person_rays_launch_matches_the_restatement(cuda, name):
    c, want = SV.rays_case_and_expected(name)
    got = MH.person_rays(_up(c['coords01'], cuda), _up(c['cov01'], cuda), _up(FR.pack_placements(c['places']), cuda).reshape(-1),
                         _up(c['single_box'], cuda), c['spec'], c['n_views'], c['weights'])
    assert got.dtype == torch.float64 and tuple(got.shape) == want.shape
    worst = SV.compare_rays(got.cpu().numpy(), want)
    print(f'{name}: {int((~np.isnan(want[..., 0])).sum())} of {want[..., 0].size} rays, worst direction deviation {worst:.2e}')


@gpu
@pytest.mark.parametrize('assignment', ['greedy', 'optimal'])
@pytest.mark.parametrize('name', list(SV.CASES))
def test_association_launch_matches_the_restatement_and_the_smoothing_launch(cuda, name, assignment):
    """The bounds of tests/test_single_view.py, the restatement's filter fed with the launch's own fp32 z and R; and
    metro_smooth_tracks on the CSR and the arrays the launch wrote leaves the working state, torch.equal."""
    c = SV.case(name)
    state, ids, next_id = _up(c['state'], cuda), _up(c['ids'], cuda), _up(np.asarray(c['next_id'], np.int32).reshape(1), cuda)
    with torch.cuda.device(cuda):
        found = MH.associate_tracks_rays(_up(c['poses'], cuda), _up(c['cov'], cuda), c['times'], c['step_rows'], c['step_starts'], state,
                                         ids, next_id, _up(c['single_box'], cuda), _up(c['rays'], cuda), c['max_cost'], c['clip'],
                                         c['min_joints'], c['max_age'], c['q'], c['r_floor'], c['cov_scale'], c['v0'], None, assignment,
                                         c['depth_sigma'])
        carried = state.clone()
        used = MH.smooth_tracks(found.poses, found.covariance, c['times'], found.rows, found.starts, 'filter', 'covariance', c['q'],
                                c['r_floor'], c['cov_scale'], c['v0'], None, carried)[3]
    got = {k: getattr(found, k).cpu().numpy() for k in ('track_index', 'track_id', 'cost', 'rows', 'starts', 'n_new', 'n_dropped',
                                                       'n_unplaced', 'poses', 'ray_depth')}
    got.update(cov=found.covariance.cpu().numpy(), working=found.working_state.cpu().numpy(), state=state.cpu().numpy(),
               ids=ids.cpu().numpy(), next_id=int(next_id.cpu()[0]))
    want = SV.associate(c, assignment, placed=(got['poses'], got['cov']))
    SV.check_margins(want, assignment)
    worst = SV.compare(got, want, c)
    placed = ~torch.isnan(found.ray_depth)
    print(f"{name}, {assignment}: {int(placed.sum())} joints placed, {want['n_unplaced']} unplaced; worst cost {worst[0]:.2e} mm, state "
          f"{worst[1]:.2e} rel, z {worst[2]:.2e} mm, tau {worst[3]:.2e} mm, R {worst[4]:.2e} rel")
    bits = lambda t: t.view(torch.int64)
    assert torch.equal(bits(carried), bits(found.working_state)), 'the smoothing launch leaves the working state, bit for bit'
    assert (used[placed] == 1).all()


def _entry(c, cuda, assignment, ray_rows):
    """One call of the C entry itself -- metro_associate_tracks_rays if `ray_rows`, else metro_associate_tracks[_optimal] -- into
    outputs pre-filled with the sentinel -> the dict assert_ray_walk_is_the_plain_walk reads."""
    import ctypes as C
    from metro_pose3d_amd import _lib
    n, nj = c['poses'].shape[:2]
    cap = len(c['ids'])
    t = {k: _up(np.asarray(c[k], dt), cuda) for k, dt in (('poses', np.float32), ('cov', np.float32), ('times', np.float64),
                                                            ('step_rows', np.int32), ('step_starts', np.int32), ('state', np.float64),
                                                            ('ids', np.int32))}
    t['next_id'] = _up(np.asarray(c['next_id'], np.int32).reshape(1), cuda)
    ints = lambda k: torch.full((k,), SV.SENTINEL, dtype=torch.int32, device=cuda)
    t.update(track_index=ints(n), track_id=ints(n), rows=ints(n), starts=ints(cap + 1), n_new=ints(1), n_dropped=ints(1), n_unplaced=ints(1),
             cost=torch.full((n,), float(SV.SENTINEL), dtype=torch.float32, device=cuda),
             ray_depth=torch.full((n, nj), float(SV.SENTINEL), dtype=torch.float32, device=cuda),
             working=torch.full((cap, nj, 28), float(SV.SENTINEL), dtype=torch.float64, device=cuda))
    p = lambda k: C.c_void_p(t[k].data_ptr())
    shared = [p('poses'), p('cov'), p('times'), n, p('step_rows'), len(c['step_rows']), p('step_starts'), len(c['step_starts']) - 1,
              C.byref(_lib.MetroSpec(n_joints_out=nj)), _lib.METRO_SMOOTH_COVARIANCE, c['q'], c['r_floor'], c['cov_scale'], c['v0'], c['gate'],
              c['max_cost'], c['clip'], c['min_joints'], c['max_age'], p('state'), cap, p('ids'), p('next_id'), p('working'),
              p('track_index'), p('track_id'), p('cost'), p('rows'), p('starts'), p('n_new'), p('n_dropped')]
    stream = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    lib = _lib.load()
    with torch.cuda.device(cuda):
        if ray_rows:
            t.update(single_box=_up(c['single_box'], cuda), rays=_up(c['rays'], cuda))
            _lib.check(lib.metro_associate_tracks_rays(*shared, int(assignment == 'optimal'), p('single_box'), p('rays'), c['depth_sigma'],
                                                       p('ray_depth'), p('n_unplaced'), stream), 'metro_associate_tracks_rays')
        else:
            name = 'metro_associate_tracks_optimal' if assignment == 'optimal' else 'metro_associate_tracks'
            _lib.check(getattr(lib, name)(*shared, stream), name)
    return {k: v.cpu().numpy() for k, v in t.items()}


@gpu
@pytest.mark.parametrize('assignment', ['greedy', 'optimal'])
@pytest.mark.parametrize('name', NO_RAY_ROW_CASES)
def test_ray_entry_without_a_ray_row_is_the_plain_entry(cuda, name, assignment):
    """metro_associate_tracks_rays with single_box all -1 and rays of NaN against metro_associate_tracks[_optimal] on the same
    inputs: every shared output, the table and the working state bit for bit, n_unplaced 0, poses and covariance untouched."""
    c = AR.CASES[name]()
    assert_ray_walk_is_the_plain_walk(_entry(without_ray_rows(c), cuda, assignment, True), _entry(c, cuda, assignment, False), c)


# ---- the whole call -------------------------------------------------------------------------------------------------------------------

def _rig():
    """3 cameras x 2 exposures: 6 frames of noise (frame = 3 step + camera); 2 boxes on each camera at the first exposure, 2 boxes
    on camera 0 alone at the second."""
    rng = np.random.default_rng(29)
    cams = TR.ring_cameras([0, 100, 215], focal=260.0, principal=(160.0, 120.0)) * 2
    frames = [rng.integers(0, 256, (240, 320, 3), dtype=np.uint8) for _ in cams]
    one = np.array([[60.0, 40, 70, 150], [170, 50, 80, 140], [50, 30, 90, 160], [180, 60, 60, 120], [90, 45, 75, 150], [200, 40, 70, 160]])
    boxes = np.concatenate([one, one[:2] + [4.0, 2.0, 0, 0]])
    fi = np.concatenate([np.repeat(np.arange(3), 2), [3, 3]])
    return cams, frames, boxes, fi, np.repeat([0.0, 0.125], 3)


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


def _by_hand(frames, boxes, path, cams, fi, stamps, tracks, precision, kw):
    """The chain follow_rig_poses_in_frames(single_view='rays') enqueues, composed from the frames module's own front end and the
    heads launches -> dict of what the call returns, and the rays."""
    from metro_pose3d_amd.inference import _engine_for
    call = FR._checked_call(frames, boxes, np.asarray(fi, np.int64), 'world', None, 'auto', precision, None, 'rgb', 'bt601', 'float32')
    device = FR._call_device(call.boxes, call.frames)
    times = FR._box_times(stamps, np.asarray(fi, np.int64), len(boxes))
    step_times, box_step = np.unique(times, return_inverse=True)
    with torch.cuda.device(device):
        eng = _engine_for(path, call.precision, device, len(boxes))
        crops, places = FR._warp_views(call.frames, cams, call.boxes, call.fi, call.vs, eng.spec.proc_side, device, call.crop_dtype)
        forward = FR._forward_coords01(eng, crops, call.check_finite, True)
        coords01, cov01, places = forward[1], forward[3][0], places.reshape(-1)
        cost, n_pairs = MH.view_affinity_steps(coords01, cov01, places, _up(np.asarray(fi, np.int32), device),
                                               _up(box_step.astype(np.int32), device), eng.spec, 1, 'covariance', 2.0, 500.0, None)
        labels, n_persons, rows, starts = MH.cluster_views(cost, kw['match_max_cost_mm'], 1)
        poses, n_rays, residual, cov = MH.triangulate_joints(coords01, cov01, places, rows, starts, eng.spec, 'covariance', 2.0, True)
        person_step, person_times, step_rows, step_starts, single = MH.person_steps_labels(labels, n_persons, box_step, step_times)
        rays = MH.person_rays(coords01, cov01, places, single, eng.spec, 1, 'covariance')
        found = MH.associate_tracks_rays(poses, cov, person_times, step_rows, step_starts, tracks.state, tracks.ids, tracks.next_id, single,
                                         rays, max_cost_mm=kw['max_cost_mm'])
        smooth = MH.smooth_tracks(found.poses, found.covariance, person_times, found.rows, found.starts, state=tracks.state)
    p = int(n_persons.cpu()[0])
    return dict(person_index=labels, cost=cost, n_pairs=n_pairs, poses=poses[:p], n_rays=n_rays[:p], residual=residual[:p],
                world_covariance=cov[:p], person_step=person_step[:p], track_index=found.track_index[:p], track_id=found.track_id[:p],
                track_cost=found.cost[:p], n_new=found.n_new, n_dropped=found.n_dropped, smoothed=tuple(t[:p] for t in smooth),
                single_view=(single >= 0).to(torch.uint8)[:p], ray_depth=found.ray_depth[:p], n_unplaced=found.n_unplaced), rays, single


def _waiting_table(rays, single, person, nj, t_last, cuda):
    """A table whose slot 0 waits exactly on the rays of `person`, 3000 mm from the camera, at rest, last seen at t_last."""
    table = FR.new_track_table(8, nj, cuda)
    state = np.zeros((8, nj, 28))
    state[..., 27] = np.nan
    r = rays[person].cpu().numpy()
    assert single[person] >= 0 and np.isfinite(r).all()
    state[0, :, :3] = r[:, :3] + 3000.0 * r[:, 3:6]
    state[0, :, 6 + np.array([0, 6, 11])] = 25.0
    state[0, :, 6 + np.array([15, 18, 20])] = 1e4
    state[0, :, 27] = t_last
    table.state.copy_(_up(state, cuda))
    table.ids[0], table.next_id[0] = 0, 1
    return table


@gpu
@pytest.mark.parametrize('precision', ['f64', 'f16'])
def test_follow_rig_poses_is_the_composition_of_the_heads_launches(cuda, tmp_path, precision):
    """A synthetic model's rays mean nothing, so the case builds the situation itself: slot 0 of the table waits on the rays of the
    first person the second exposure shows (taken from heads.person_rays' own output) 3000 mm out, and max_cost_mm is 5 mm, so
    that nothing else continues it.  That person's ray row must match at a cost of about 0 and be placed at tau = 3000."""
    from tests.test_gpu_placement import _toy_engine_model
    spec, _, path = _toy_engine_model(tmp_path)
    nj = spec.skeleton.n_out
    cams, frames, boxes, fi, stamps = _rig()
    kw = dict(match_max_cost_mm=600.0, max_cost_mm=5.0, precision=precision, capacity=8)
    _, rays, single = _by_hand(frames, boxes, path, cams, fi, stamps, FR.new_track_table(8, nj, cuda), precision, kw)
    single = single.cpu().numpy()
    waiting = lambda: _waiting_table(rays, single, person, nj, 0.125 - 1.0 / 32.0, cuda)
    first = FR.follow_rig_poses_in_frames(frames, boxes, path, cams, fi, stamps, **kw)
    late = first.person_index[6:].cpu().numpy()
    assert len(set(late.tolist())) == 2 and all(int(first.single_view[p]) == 1 for p in late), \
        'two boxes of one frame are two persons, each seen by one camera'
    person = int(late[0])
    want, _, _ = _by_hand(frames, boxes, path, cams, fi, stamps, waiting(), precision, kw)
    got = FR.follow_rig_poses_in_frames(frames, boxes, path, cams, fi, stamps, tracks=waiting(), **kw)
    for k in ('person_index', 'cost', 'n_pairs', 'world_covariance', 'person_step', 'track_index', 'track_id', 'track_cost', 'n_new',
              'n_dropped', 'single_view', 'ray_depth', 'n_unplaced'):
        assert _same(getattr(got, k), want[k]), k
    for k in ('poses', 'n_rays', 'residual'):
        assert _same(getattr(got.world, k), want[k]), k
    assert _same(tuple(got.smoothed[:4]), want['smoothed'])
    # the situation: the ray row continues slot 0 at about no cost and is placed 3000 mm out; the world poses stay the triangulation's
    assert int(got.track_index[person]) == 0 and int(got.track_id[person]) == 0 and float(got.track_cost[person]) < 1e-3
    depth = got.ray_depth[person]
    assert (torch.abs(depth - 3000.0) < 1.0).any() and torch.isnan(got.world.poses[person]).all()
    assert torch.isnan(got.world_covariance[person]).all() and int(got.person_step[person]) == 1
    assert torch.isfinite(got.smoothed.poses[person]).all() and (got.smoothed.used[person] == 1).any()
    assert int(got.single_view.sum()) >= 2 and int(got.n_unplaced) == int(got.single_view.sum()) - int((got.track_index[got.single_view == 1] >= 0).sum())
    # cut in two at the step boundary
    tracks, parts = waiting(), []
    for t in (0, 1):
        sel = fi // 3 == t
        part = FR.follow_rig_poses_in_frames(frames[3 * t:3 * t + 3], boxes[sel], path, cams[3 * t:3 * t + 3], fi[sel] - 3 * t,
                                             stamps[3 * t:3 * t + 3], tracks=tracks, **kw)
        tracks = part.tracks
        parts.append(part)
    for k in ('track_id', 'track_index', 'track_cost', 'single_view', 'ray_depth'):
        assert _same(torch.cat([getattr(p, k) for p in parts]), getattr(got, k)), k
    assert _same(tuple(tracks), tuple(got.tracks)) and int(parts[0].n_unplaced) + int(parts[1].n_unplaced) == int(got.n_unplaced)
    print(f'{precision}: persons {len(got.person_step)}, single {got.single_view.tolist()}, ids {got.track_id.tolist()}, placed '
          f'{int((~torch.isnan(depth)).sum())} of {nj} joints at tau {float(depth[~torch.isnan(depth)].min()):.3f} .. '
          f'{float(depth[~torch.isnan(depth)].max()):.3f}, cost {float(got.track_cost[person]):.2e} mm, unplaced {int(got.n_unplaced)}')


@gpu
@pytest.mark.parametrize('precision', ['f64', 'f16'])
def test_single_view_skip_is_follow_world_poses_in_frames(cuda, tmp_path, precision):
    from tests.test_gpu_placement import _toy_engine_model
    _, _, path = _toy_engine_model(tmp_path)
    cams, frames, boxes, fi, stamps = _rig()
    kw = dict(match_max_cost_mm=600.0, max_cost_mm=590.0, precision=precision, capacity=8)
    world = FR.follow_world_poses_in_frames(frames, boxes, path, cams, fi, stamps, **kw)
    rig = FR.follow_rig_poses_in_frames(frames, boxes, path, cams, fi, stamps, single_view='skip', **kw)
    for k in FR.FollowedWorldPoses._fields:
        assert _same(tuple(getattr(rig, k)) if isinstance(getattr(rig, k), tuple) else getattr(rig, k),
                     tuple(getattr(world, k)) if isinstance(getattr(world, k), tuple) else getattr(world, k)), k
    p = len(world.person_step)
    assert rig.single_view.dtype == torch.uint8 and tuple(rig.single_view.shape) == (p,) and int(rig.single_view.sum()) == 0
    assert rig.ray_depth.dtype == torch.float32 and tuple(rig.ray_depth.shape) == (p, world.smoothed.poses.shape[1])
    assert torch.isnan(rig.ray_depth).all() and rig.n_unplaced.tolist() == [0] and (world.person_step[-2:] == -1).all()
