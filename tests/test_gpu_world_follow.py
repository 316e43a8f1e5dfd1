"""metro_view_affinity_steps, metro_triangulate_joints_cov, metro_person_steps and frames.follow_world_poses_in_frames on the
MI355X: the three launches against their fp64 restatement (tests/world_follow_ref.py) into poisoned output buffers, the plain
entries bit for bit, and the whole call against the composition by hand of the calls it joins.  The argument checks at the end
run before any launch."""
import dataclasses

import numpy as np
import pytest
import torch

from metro_pose3d_amd import ModelSpec, frames as FR, heads as MH
from metro_pose3d_amd.joints import Skeleton
from tests import match_views_ref as MR
from tests import triangulation_ref as TR
from tests import world_follow_ref as WR

H36M = ModelSpec(50, 32, 'h36m')
gpu = pytest.mark.gpu


class _JointSpec:
    """H36M's geometry with a made-up skeleton of n_out joints (pairs l*/r* and a centre joint if n_out is odd), the head in a
    scrambled order: the launches read the joint counts, the permutation and the mirror table only."""

    def __init__(self, n_out, seed):
        names = [f'{side}j{k}' for k in range(n_out // 2) for side in 'lr'] + ['cj'] * (n_out % 2)
        perm = np.random.default_rng(seed).permutation(n_out)
        head = [None] * n_out
        for i, h in enumerate(perm):
            head[h] = names[i]
        self.skeleton = Skeleton(tuple(head), tuple(int(h) for h in perm), tuple(names), ())
        for f in dataclasses.fields(H36M):
            if f.name != 'skeleton':
                setattr(self, f.name, getattr(H36M, f.name))

    def to_c(self, precision):
        cs = H36M.to_c(precision)
        cs.n_joints_head = cs.n_joints_out = self.skeleton.n_out
        for i, p in enumerate(self.skeleton.permutation):
            cs.permutation[i] = p
        return cs


def _up(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _device_case(c, cuda):
    return dict(coords01=_up(c['coords01'], cuda), cov01=_up(c['cov01'], cuda), places=_up(FR.pack_placements(c['places']), cuda).reshape(-1))


# ---- the three launches ------------------------------------------------------------------------------------------------------

def _affinity_case(n):
    from tests.test_gpu_match_views import _n65, _n128
    return {2: MR.CASES['rig-2x1'], 65: _n65, 128: _n128}[n](H36M, 'covariance')


@gpu
@pytest.mark.parametrize('n', [2, 65, 128])
def test_gated_affinity_matches_the_restatement_and_the_plain_entry(cuda, n):
    c = _affinity_case(n)
    assert len(c['fi']) == n
    d = _device_case(c, cuda)
    tail = (H36M, c['n_views'], c['weights'], c['min_angle_deg'], c['clip_mm'], c['min_joints'])
    gated = lambda step_index: MH.view_affinity_steps(d['coords01'], d['cov01'], d['places'], c['fi'], step_index, *tail)
    plain = MH.view_affinity(d['coords01'], d['cov01'], d['places'], c['fi'], *tail)
    same = gated(np.full(n, 3, np.int32))
    assert torch.equal(same[0], plain[0]) and torch.equal(same[1], plain[1]), 'an all-equal step index is the plain entry'
    step = (np.arange(n) % 2).astype(np.int32)
    if n == 2:
        step[:] = [0, 0]                                    # two boxes, two steps would leave nothing to compare
    got = gated(_up(step, cuda))
    other = _up(step[:, None] != step[None, :], cuda)
    assert torch.equal(got[0][~other], plain[0][~other]) and torch.equal(got[1][~other], plain[1][~other]), 'same-step pairs'
    assert torch.isposinf(got[0][other]).all() and (got[1][other] == 0).all()
    worst = MR.compare((got[0].cpu().numpy(), got[1].cpu().numpy()), WR.gated(*MR.expected(c, H36M), step), MR.PARITY_MM)
    print(f'{n} boxes, 2 steps: worst cost deviation {worst:.2e} mm vs the fp64 restatement')
    if n == 2:
        two = gated([0, 1])
        assert torch.isposinf(two[0]).all() and (two[1] == 0).all()


@gpu
@pytest.mark.parametrize('persons,n_out', [(3, 21), (5, 13), (16, 17)], ids=['63-threads', '65-threads', '272-threads'])
@pytest.mark.parametrize('weights', ['uniform', 'covariance'])
def test_covariance_launch_matches_the_restatement_and_the_plain_entry(cuda, persons, n_out, weights):
    spec = H36M if n_out == 17 else _JointSpec(n_out, seed=n_out)
    sk = spec.skeleton
    rng = np.random.default_rng(persons)
    s = TR.ring_scene([0, 75, 160, 250], persons, spec, seed=40 + persons)
    m, lrc = len(s['boxes']), TR.pixel_scale(spec)[0]
    coords01 = s['coords01'].copy()
    coords01[..., :2] += rng.normal(0, 2.0 / lrc, (m, sk.n_head, 2)).astype(np.float32)
    coords01[1, sk.permutation[2]] = np.nan                 # one ray less for a joint of person 0
    groups = FR.person_groups(s['pi'], s['fi'])
    rows, starts = groups[0].copy(), groups[1].copy()
    starts[-1] -= 3                                          # the last person keeps one row: undetermined, a NaN block
    c = TR.case(coords01, TR.cov01_for(rng.uniform(0.5, 30.0, (m, sk.n_head)), spec, (m, sk.n_head)), s['places'], rows, starts, weights)
    d = _device_case(c, cuda)
    args = (d['coords01'], d['cov01'], d['places'], c['rows'], c['starts'], spec, weights)
    plain = MH.triangulate_joints(*args)
    points, n_rays, residual, cov = MH.triangulate_joints(*args, return_covariance=True)
    bits = lambda t: t.view(torch.int32)                    # torch.equal on the bit patterns: NaN equals NaN
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip((points, n_rays, residual), plain)), 'the plain entry, bit for bit'
    assert cov.shape == (persons, n_out, 9) and cov.dtype == torch.float32
    got = tuple(t.cpu().numpy() for t in (points, n_rays, residual))
    TR.compare(got, TR.expected(c, spec), TR.PARITY_MM)
    want, det = WR.covariance(c, spec)
    solved = ~np.isnan(got[0]).any(axis=-1)
    assert solved[:-1].all() and not solved[-1].any() and (det[solved] >= TR.min_det(2.0)).all()
    worst = WR.compare_covariance(cov.cpu().numpy(), want, got[0])
    print(f'{persons} x {n_out}, {weights}: worst covariance deviation {worst:.2e} of the largest entry, smallest det A~ {np.nanmin(det):.3g}')


@gpu
@pytest.mark.parametrize('name', [k for k in WR.person_steps_cases() if k in ('n1-s1', 'n64-s2', 'n65-s65', 'n128-s2', 'n128-s65',
                                                                            'n128-s1', 'descending', 'rows-out-of-range',
                                                                            'steps-out-of-range', 'count-below-n-garbage', 'views-2')])
def test_person_steps_launch_matches_the_restatement(cuda, name):
    c = WR.person_steps_cases()[name]
    got = MH.person_steps(_up(c['rows'], cuda), _up(c['starts'], cuda), _up(np.asarray([c['n_persons']], np.int32), cuda),
                          c['box_step'], c['step_times'], c['n_views'])
    assert [t.dtype for t in got] == [torch.int32, torch.float64, torch.int32, torch.int32]
    WR.compare_person_steps([t.cpu().numpy() for t in got], WR.person_steps(**c))


# ---- the whole call ----------------------------------------------------------------------------------------------------------

def _rig():
    """3 cameras x 2 exposures: 6 frames of noise (frame = 3 step + camera), 2 boxes on each, step-major."""
    rng = np.random.default_rng(23)
    cams = TR.ring_cameras([0, 100, 215], focal=260.0, principal=(160.0, 120.0)) * 2
    frames = [rng.integers(0, 256, (240, 320, 3), dtype=np.uint8) for _ in cams]
    one = np.array([[60.0, 40, 70, 150], [170, 50, 80, 140], [50, 30, 90, 160], [180, 60, 60, 120], [90, 45, 75, 150], [200, 40, 70, 160]])
    boxes = np.concatenate([one, one + [4.0, 2.0, 0, 0]])
    fi = np.repeat(np.arange(6), 2)
    return cams, frames, boxes, fi, np.repeat([0.0, 0.125], 3)


def _equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)


@gpu
@pytest.mark.parametrize('precision', ['f64', 'f16'])
def test_follow_world_poses_is_the_composition_of_the_calls_it_joins(cuda, tmp_path, precision):
    """A synthetic model's poses mean nothing, so this checks plumbing and equivalence, with thresholds above the clips so that
    boxes do merge and tracks do continue: the world poses are match_poses_in_frames' per step; the tracks are
    heads.associate_tracks and heads.smooth_tracks on the world poses and covariance the call returned, with the steps built on
    the host; the call cut in two at the step boundary gives the same ids and, per id, the same state."""
    from tests.test_gpu_placement import _toy_engine_model
    spec, _, path = _toy_engine_model(tmp_path)
    sk = spec.skeleton
    cams, frames, boxes, fi, stamps = _rig()
    kw = dict(match_max_cost_mm=600.0, max_cost_mm=590.0, precision=precision, capacity=8)
    got = FR.follow_world_poses_in_frames(frames, boxes, path, cams, fi, stamps, **kw)
    labels = got.person_index.cpu().numpy()
    persons = int(labels.max()) + 1
    assert got.world.poses.shape == (persons, sk.n_out, 3) and got.world_covariance.shape == (persons, sk.n_out, 9)
    assert got.track_index.shape == (persons,) and got.smoothed.poses.shape == (persons, sk.n_out, 3)
    step_of_box = fi // 3
    assert all(len(set(step_of_box[labels == p])) == 1 for p in range(persons)), 'no person spans two steps'
    # the world poses: match_poses_in_frames per step
    parts = []
    for t in (0, 1):
        sel = step_of_box == t
        part = FR.match_poses_in_frames(frames[3 * t:3 * t + 3], boxes[sel], path, cams[3 * t:3 * t + 3], fi[sel] - 3 * t, max_cost_mm=600.0,
                                        precision=precision)
        parts.append(part)
        assert _equal(part.cost, got.cost[torch.from_numpy(sel).to(cuda)][:, torch.from_numpy(sel).to(cuda)])
    for field in ('poses', 'n_rays', 'residual'):
        assert _equal(torch.cat([getattr(p.world, field) for p in parts]), getattr(got.world, field)), field
    assert _equal(torch.cat([parts[0].person_index, parts[1].person_index + len(parts[0].world.poses)]), got.person_index)
    nan = torch.isnan(got.world.poses).any(dim=-1)
    assert torch.equal(torch.isnan(got.world_covariance).all(dim=-1), nan) and torch.isfinite(got.world.poses).any()
    # the tracks: the steps on the host (persons with company have a step), then the two heads calls
    sizes = np.bincount(labels, minlength=persons)
    lowest = np.array([np.flatnonzero(labels == p)[0] for p in range(persons)])
    person_step = np.where(sizes >= 2, step_of_box[lowest], -1).astype(np.int32)
    assert np.array_equal(got.person_step.cpu().numpy(), person_step) and (sizes >= 2).any()
    listed = np.flatnonzero(person_step >= 0)
    times = np.where(person_step >= 0, np.array([0.0, 0.125])[person_step], np.nan)
    step_rows, step_starts = FR.time_steps(times[listed])
    table = FR.new_track_table(8, sk.n_out, cuda)
    with torch.cuda.device(cuda):
        found = MH.associate_tracks(got.world.poses, got.world_covariance, times, listed[step_rows], step_starts, table.state, table.ids,
                                    table.next_id, max_cost_mm=590.0)
        smooth = MH.smooth_tracks(got.world.poses, got.world_covariance, times, found.rows, found.starts, state=table.state)
    assert _equal(found.track_index, got.track_index) and _equal(found.track_id, got.track_id) and _equal(found.cost, got.track_cost)
    assert _equal(found.n_new, got.n_new) and _equal(found.n_dropped, got.n_dropped)
    assert _equal(table.state, got.tracks.state) and _equal(table.ids, got.tracks.ids) and _equal(table.next_id, got.tracks.next_id)
    for a, b in zip(smooth, got.smoothed[:4]):
        assert _equal(a, b)
    assert got.smoothed.state is got.tracks.state and (got.track_id >= 0).any()
    # cut in two at the step boundary
    tracks, ids = None, []
    for t in (0, 1):
        sel = step_of_box == t
        part = FR.follow_world_poses_in_frames(frames[3 * t:3 * t + 3], boxes[sel], path, cams[3 * t:3 * t + 3], fi[sel] - 3 * t,
                                               stamps[3 * t:3 * t + 3], tracks=tracks, **kw)
        tracks = part.tracks
        ids.append(part.track_id)
    assert _equal(torch.cat(ids), got.track_id)
    assert _equal(tracks.ids, got.tracks.ids) and _equal(tracks.state, got.tracks.state) and _equal(tracks.next_id, got.tracks.next_id)
    print(f'{precision}: {persons} persons of {len(boxes)} boxes, sizes {sizes.tolist()}, ids {got.track_id.tolist()}, '
          f'new {int(got.n_new)}, dropped {int(got.n_dropped)}')


# ---- the argument checks: before any launch, no GPU needed -----------------------------------------------------------------------

def test_follow_world_poses_checks_its_arguments_before_any_launch():
    cams = TR.ring_cameras([0, 90])
    frames = [np.zeros((8, 8, 3), np.uint8)] * 2
    boxes = [[0, 0, 4, 4], [1, 1, 4, 4]]
    call = lambda boxes=boxes, cameras=cams, fi=(0, 1), ts=(0.0, 0.0), **kw: FR.follow_world_poses_in_frames(
        frames, boxes, 'no-such-model.npz', cameras, fi, ts, **kw)
    with pytest.raises(ValueError, match='at most 128'):
        call(boxes=np.tile([0.0, 0, 4, 4], (129, 1)), fi=np.arange(129) % 2)
    with pytest.raises(ValueError, match='calibrated cameras'):
        call(cameras=None)
    with pytest.raises(ValueError, match='one value per box'):
        call(fi=(0,))
    with pytest.raises(ValueError, match='timestamps must hold one value per box'):
        call(ts=(0.0,), fi=(0, 1))
    with pytest.raises(ValueError, match='timestamps must hold one value per box'):
        call(boxes=np.tile([0.0, 0, 4, 4], (4, 1)), fi=(0, 1, 0, 1), ts=(0.0,))
    for bad in (float('nan'), float('inf')):
        with pytest.raises(ValueError, match='finite'):
            call(ts=(0.0, bad))
    for bad in (0, 129, -1, 2.5, True):
        with pytest.raises(ValueError, match='capacity'):
            call(capacity=bad)
    with pytest.raises(ValueError, match='tracks must be'):
        call(tracks=(1, 2, 3))
    with pytest.raises(ValueError, match='at most 64'):
        call(boxes=np.tile([0.0, 0, 4, 4], (65, 1)), cameras=cams * 33, fi=np.arange(65), ts=np.zeros(65))
    for kw, word in ((dict(weights='robust'), 'weights'), (dict(min_angle_deg=0), 'min_angle_deg'), (dict(match_max_cost_mm=0), 'max_cost_mm'),
                     (dict(match_clip_mm=-1), 'clip_mm'), (dict(max_cost_mm=float('nan')), 'max_cost_mm'), (dict(max_age_s=-1), 'max_age_s'),
                     (dict(mode='rts'), 'mode'), (dict(gate=-1), 'gate'), (dict(min_joints=0), 'min_joints')):
        with pytest.raises(ValueError, match=word):
            call(**kw)
    # heads: checked before the library or a device is touched
    m, nj = 4, H36M.skeleton.n_head
    c01, cov, places = torch.zeros((m, nj, 3)), torch.zeros((m, nj, 6)), torch.zeros(m * 208, dtype=torch.uint8)
    with pytest.raises(ValueError, match='step_index must hold one value per box'):
        MH.view_affinity_steps(c01, cov, places, [0, 1, 2, 3], [0, 1], H36M)
    with pytest.raises(ValueError, match='device tensors'):
        MH.person_steps([0], [0, 1], [1], [0], [0.0])
    with pytest.raises(ValueError, match='at most'):
        MH.person_steps(torch.zeros(0, dtype=torch.int32), torch.zeros(130, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), [], [])
