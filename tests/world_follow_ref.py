"""fp64 NumPy restatement of what follow_world_poses_in_frames adds to the tree (include/metro_hip.h): the covariance of
metro_triangulate_joints_cov, the step gate of metro_view_affinity_steps, metro_person_steps, and the chain of the six launches.
TEST INFRASTRUCTURE: the product never imports it.  The covariance is np.linalg.inv of the dense 3x3 A where the kernel has
cofactors, the person steps are a Python sort of (step, person) tuples where the kernel counts ranks, and the gated matrix is
tests/match_views_ref.py's with +inf written where the steps differ.  Affinity, clustering, triangulation, association and
smoothing are the existing restatements, imported."""
from __future__ import annotations

import functools

import numpy as np

from tests import follow_tracks_ref as FT
from tests import match_views_ref as MR
from tests import track_smoothing_ref as TS
from tests import triangulation_ref as TR

COVARIANCE_REL = TS.COVARIANCE_REL         # 1e-6 of the block's largest entry: the smoothing tests' bound for covariance blocks
SENTINEL = -7


# ---- metro_triangulate_joints_cov -----------------------------------------------------------------------------------------------

def covariance(c, spec):
    """The covariance blocks of a triangulation case (TR.case) -> (cov float64 [P, Jout, 9], NaN where the joint is undetermined;
    det float64 [P, Jout]: det A~ of the final solve, NaN where there is none)."""
    sk, q = spec.skeleton, c['places']
    lrc, _ = TR.pixel_scale(spec)
    d, o, head, ok = TR.rays(c['coords01'], q.inv_intrinsics, q.rot_to_world, q.cam_loc, sk.permutation, sk.out_mirror, spec)
    m, n_out = ok.shape
    rows, starts = np.asarray(c['rows'], np.int64), np.asarray(c['starts'], np.int64)
    n_persons = len(starts) - 1
    weighted = c['weights'] == TR.COVARIANCE
    threshold = TR.min_det(c['min_angle_deg'])
    cov = np.full((n_persons, n_out, 9), np.nan)
    det = np.full((n_persons, n_out), np.nan)
    if weighted:
        scale = lrc ** 2 * np.asarray(q.inv_intrinsics, np.float32).astype(np.float64).reshape(-1, 3, 3)[:, 0, 0] ** 2
        c01 = np.asarray(c['cov01'], np.float32).astype(np.float64)
    for p in range(n_persons):
        group = rows[max(starts[p], 0):min(starts[p + 1], len(rows))]
        group = group[(group >= 0) & (group < m)]
        for r in range(n_out):
            use = group[ok[group, r]]
            dd, oo, w = d[use, r], o[use], np.ones(len(use))
            x = TR._solve(dd, oo, w, threshold)
            if x is not None and weighted:
                z = np.einsum('ka,ka->k', dd, x[None] - oo)
                s2 = 0.5 * (c01[use, head[use, r], 0] + c01[use, head[use, r], 1]) * scale[use]
                s2 = np.maximum(s2, 1e-12 * scale[use])
                with np.errstate(invalid='ignore', divide='ignore'):
                    w = 1.0 / (s2 * z * z)
                keep = (z > 0) & np.isfinite(w)
                dd, oo, w = dd[keep], oo[keep], w[keep]
                x = TR._solve(dd, oo, w, threshold)
            if x is None:
                continue
            a = (w[:, None, None] * (np.eye(3)[None] - dd[:, :, None] * dd[:, None, :])).sum(axis=0)
            det[p, r] = np.linalg.det(a / w.sum())
            s2 = 1.0
            if not weighted:
                v = x[None] - oo
                perp = v - dd * np.einsum('ka,ka->k', dd, v)[:, None]
                s2 = (perp ** 2).sum() / (2 * len(dd) - 3)
            cov[p, r] = (s2 * np.linalg.inv(a)).reshape(9)
    return cov, det


def compare_covariance(got, want, points):
    """fp32 blocks of the code under test against the restatement's: NaN exactly where the points are NaN, every other block
    within COVARIANCE_REL of its largest entry (an all-zero block: exactly zero).  -> the worst relative deviation."""
    got, want, points = np.asarray(got), np.asarray(want), np.asarray(points)
    assert got.dtype == np.float32 and got.shape == want.shape
    nan = np.isnan(points).any(axis=-1)
    assert np.array_equal(np.isnan(got).all(axis=-1), nan) and np.array_equal(np.isnan(got).any(axis=-1), nan)
    assert np.array_equal(np.isnan(want).any(axis=-1), nan)
    worst = 0.0
    for g, w in zip(got[~nan].astype(np.float64), want[~nan]):
        scale = np.abs(w).max()
        if scale == 0:
            assert (g == 0).all()
            continue
        worst = max(worst, float(np.abs(g - w).max() / scale))
    assert worst <= COVARIANCE_REL, worst
    return worst


# ---- metro_view_affinity_steps --------------------------------------------------------------------------------------------------

def gated(cost, n_pairs, step_index):
    """MR.affinity's outputs with +inf / 0 written where the steps of the two boxes differ."""
    step = np.asarray(step_index).reshape(-1)
    other = step[:, None] != step[None, :]
    return np.where(other, np.float32(np.inf), cost).astype(np.float32), np.where(other, 0, n_pairs).astype(np.int32)


# ---- metro_person_steps ---------------------------------------------------------------------------------------------------------

def person_steps(rows, starts, n_persons, n, n_views, box_step, step_times):
    """-> (person_step int32 [n], person_times float64 [n], step_rows int32 [n], step_starts int32 [S + 1])."""
    rows, starts, box_step = (np.asarray(a, np.int64).reshape(-1) for a in (rows, starts, box_step))
    step_times = np.asarray(step_times, np.float64).reshape(-1)
    n_steps = len(step_times)
    person_step = np.full(n, -1, np.int32)
    for p in range(min(max(int(n_persons), 0), n)):
        group = rows[max(starts[p], 0):min(starts[p + 1], len(rows))]
        steps = [int(box_step[r // n_views]) for r in group if 0 <= r < len(box_step) * n_views]
        steps = [s for s in steps if 0 <= s < n_steps]
        if steps:
            person_step[p] = min(steps)
    order = sorted((int(person_step[p]), p) for p in range(n) if person_step[p] >= 0)
    step_rows = np.full(n, -1, np.int32)
    step_rows[:len(order)] = [p for _, p in order]
    step_starts = np.asarray([sum(s < k for s, _ in order) for k in range(n_steps + 1)], np.int32)
    person_times = np.array([step_times[s] if s >= 0 else np.nan for s in person_step], np.float64)
    return person_step, person_times, step_rows, step_starts


def person_steps_cases():
    """name -> dict(rows, starts, n_persons, n, n_views, box_step, step_times): the inputs of metro_person_steps."""
    cases = {}

    def case(groups, n, n_views, box_step, n_steps, n_persons=None, garbage=False, rows_extra=()):
        """groups: the boxes of each person (in person order); rows i n_views + v of them, -1 past the end."""
        rows, starts = [], [0]
        for g in groups:
            rows += [b * n_views + v for b in g for v in range(n_views)]
            starts.append(len(rows))
        count = len(groups) if n_persons is None else n_persons
        starts += [len(rows)] * (n - len(groups))
        rows += list(rows_extra) + [-1] * (n * n_views - len(rows) - len(rows_extra))
        if garbage:                                        # what lies past the count is not read
            starts[count + 1:] = [10 ** 6 + k for k in range(len(starts) - count - 1)]
        return dict(rows=np.asarray(rows, np.int32), starts=np.asarray(starts, np.int32), n_persons=count, n=n, n_views=n_views,
                    box_step=np.asarray(box_step, np.int32), step_times=np.arange(n_steps) / 32.0 + 5.0)

    cases['count-0'] = case([], 4, 1, [0, 1, 0, 1], 2)
    cases['count-1'] = case([[0, 1]], 2, 1, [0, 0], 1)
    cases['count-n'] = case([[0, 1], [2, 3]], 2, 1, [1, 1, 0, 0], 2)     # as many persons as the upper bound, all with a step
    cases['singles'] = case([[], [], []], 3, 1, [0, 1, 2], 3)            # count n, every group empty
    cases['count-below-n-garbage'] = case([[0, 2], [1, 3]], 6, 1, [1, 1, 0, 0, 1, 0], 2, garbage=True)
    cases['descending'] = case([[0, 4], [1, 5], [2, 6], [3, 7]], 8, 1, [3, 2, 1, 0, 3, 2, 1, 0], 4)
    cases['empty-step'] = case([[0, 1], [2, 3]], 4, 1, [0, 0, 2, 2], 3)
    cases['ungated'] = case([[0, 1, 2], [3, 4]], 5, 1, [2, 1, 2, 0, 1], 3)
    cases['views-2'] = case([[1, 2], [0, 3]], 4, 2, [1, 0, 0, 1], 2)
    cases['mixed'] = case([[0, 3], [], [1, 2], []], 6, 1, [1, 0, 0, 1, 0, 1], 2)
    bad = case([[0, 1], [2, 3]], 4, 1, [0, 0, 1, 1], 2)
    bad['rows'] = np.asarray([-5, 1, 400, 2], np.int32)   # person 0: {-5, 1}, person 1: {400, 2}: the bad rows are skipped
    bad['starts'] = np.asarray([-2, 2, 4, 4, 9], np.int32)
    cases['rows-out-of-range'] = bad
    bad_step = case([[0, 1], [2, 3]], 4, 1, [7, -1, 1, 1], 2)          # person 0 has no box with a step in range: -1
    cases['steps-out-of-range'] = bad_step
    rng = np.random.default_rng(5)
    for n, n_steps in ((1, 1), (64, 2), (65, 65), (128, 2), (128, 65), (128, 1)):
        # n boxes in pairs (box 2 k and 2 k + 1 one person), the persons' steps drawn at random
        steps = rng.integers(0, n_steps, n // 2)
        groups = [[2 * k, 2 * k + 1] for k in range(n // 2)]
        cases[f'n{n}-s{n_steps}'] = case(groups, n, 1, np.repeat(steps, 2).tolist() + [0] * (n % 2), n_steps)
    return cases


def compare_person_steps(got, want):
    for g, w, name in zip(got, want, ('person_step', 'person_times', 'step_rows', 'step_starts')):
        g, w = np.asarray(g).reshape(-1), np.asarray(w).reshape(-1)
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w, equal_nan=name == 'person_times'), (name, g, w)


# ---- the chain on a synthetic rig -----------------------------------------------------------------------------------------------

def walking_scene(spec, angles=(0, 90, 180, 270), n_steps=8, seed=3):
    """Two persons of nearly the same build (joint clouds within 30 mm of each other) walking through each other in front of a
    ring of cameras at 4.5 m (TR.ring_cameras): their centres pass each other between steps 3 and 4.  Boxes step-major, then
    camera-major, scrambled within each step; exact projections of the joints through every crop's own virtual camera.
    -> dict(cams (one per frame = step x camera), boxes, fi, pi, step [n], times [n], truth [S, 2, Jout, 3], places, coords01)."""
    from metro_pose3d_amd import frames as FR
    rng = np.random.default_rng(seed)
    sk = spec.skeleton
    rig = TR.ring_cameras(list(angles))
    cloud = rng.uniform(-300, 300, (sk.n_out, 3))
    clouds = (cloud, cloud + rng.uniform(-30, 30, (sk.n_out, 3)))
    base = np.array([200.0, -300.0, 1000.0])
    centre = lambda p, t: base + (np.array([-525.0 + 150.0 * t, 40.0, 0.0]) if p == 0 else np.array([175.0 - 50.0 * t, -40.0, 0.0]))
    truth = np.array([[centre(p, t) + clouds[p] for p in range(2)] for t in range(n_steps)])
    cams, boxes, fi, pi, step = [], [], [], [], []
    for t in range(n_steps):
        here = []
        for c, cam in enumerate(rig):
            cams.append(cam)
            for p in range(2):
                xc = (truth[t, p] - cam.t.astype(np.float64)) @ cam.R.astype(np.float64).T
                px = xc[:, :2] / xc[:, 2:] @ cam.intrinsic_matrix[:2, :2].astype(np.float64).T + cam.intrinsic_matrix[:2, 2]
                lo, hi = px.min(axis=0) - 30, px.max(axis=0) + 30
                here.append(([lo[0], lo[1], hi[0] - lo[0], hi[1] - lo[1]], t * len(rig) + c, p))
        for k in rng.permutation(len(here)):
            boxes.append(here[k][0]), fi.append(here[k][1]), pi.append(here[k][2]), step.append(t)
    boxes, fi, pi, step = np.array(boxes), np.array(fi), np.array(pi), np.array(step, np.int32)
    places = FR.placement_params(cams, boxes, fi, spec.proc_side)
    coords01 = np.zeros((len(boxes), sk.n_head, 3), np.float32)
    perm = np.asarray(sk.permutation)
    for i in range(len(boxes)):
        coords01[i, perm, :2] = TR.project(truth[step[i], pi[i]], places.inv_intrinsics[i], places.rot_to_world[i],
                                           places.cam_loc[i], spec).astype(np.float32)
    return dict(cams=cams, boxes=boxes, fi=fi, pi=pi, step=step, times=step / 32.0, truth=truth, places=places, coords01=coords01,
                cov01=TR.cov01_for(rng.uniform(0.5, 4.0, (len(boxes), sk.n_head)), spec, (len(boxes), sk.n_head)))


def chain(s, spec, boxes, table, weights='covariance', mode='smooth', match_max_cost=MR.MAX_COST_MM, **params):
    """The six launches restated on the boxes `boxes` (indices into the scene s) with the track table `table` = (state, ids,
    next_id) -> dict(person_index, cost, n_pairs, n_persons, points, n_rays, residual, cov, person_step, assoc (FT.associate's
    dict), smoothed (TS.smooth_tracks' tuple), table: the table after the call -- its state is the association's working state,
    which the smoothing launch leaves in the table bit for bit; the smoothing restatement keeps P as a dense matrix over a
    group's rows where the one-row steps of FT.associate pack its upper triangle, so its own state agrees to rounding only)."""
    sk = spec.skeleton
    boxes = np.asarray(boxes)
    n = len(boxes)
    places = TR._take(s['places'], boxes)
    c = dict(coords01=s['coords01'][boxes], cov01=s['cov01'][boxes], places=places, fi=s['fi'][boxes], n_views=1, weights=weights,
             min_angle_deg=2.0, clip_mm=MR.CLIP_MM, min_joints=None)
    step_times, box_step = np.unique(s['times'][boxes], return_inverse=True)
    cost, n_pairs = gated(*MR.expected(c, spec), box_step)
    person_index, n_persons, rows, starts = MR.cluster(cost, match_max_cost)
    tri = TR.case(c['coords01'], c['cov01'], places, rows, starts, weights)
    points, n_rays, residual = TR.expected(tri, spec)
    cov = covariance(tri, spec)[0].astype(np.float32)
    person_step, person_times, step_rows, step_starts = person_steps(rows, starts, n_persons, n, 1, box_step, step_times)
    a = dict(FT.DEFAULTS, poses=points, cov=cov, times=person_times, step_rows=step_rows, step_starts=step_starts, state=table[0],
             ids=table[1], next_id=table[2], min_joints=(sk.n_out + 1) // 2)
    a.update(params)
    assoc = FT.associate(a)
    smoothed = TS.smooth_tracks(points, cov, person_times, assoc['rows'], assoc['starts'], mode, a['measurement'], a['q'], a['r_floor'],
                                a['cov_scale'], a['v0'], a['gate'], assoc['state'])
    return dict(person_index=person_index, cost=cost, n_pairs=n_pairs, n_persons=n_persons, points=points, n_rays=n_rays,
                residual=residual, cov=cov, person_step=person_step, assoc=assoc, smoothed=smoothed,
                table=(assoc['working'], assoc['ids'], np.asarray([assoc['next_id']], np.int32)))


@functools.lru_cache(maxsize=None)
def _walking_scene(arch):
    from metro_pose3d_amd import ModelSpec
    spec = ModelSpec(*arch)
    return spec, walking_scene(spec)


@functools.lru_cache(maxsize=None)
def walking_in_calls(steps_per_call, arch=(50, 32, 'h36m')):
    """The walking scene in calls of `steps_per_call` steps with the table carried -> (scene, [(boxes, chain result)]), computed
    once per session: treat it as read-only."""
    spec, s = _walking_scene(arch)
    table = FT.new_table(8, spec.skeleton.n_out)
    out = []
    n_steps = int(s['step'].max()) + 1
    for t in range(0, n_steps, steps_per_call):
        boxes = np.flatnonzero((s['step'] >= t) & (s['step'] < t + steps_per_call))
        out.append((boxes, chain(s, spec, boxes, table)))
        table = out[-1][1]['table']
    return s, out
