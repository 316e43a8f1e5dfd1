"""fp64 NumPy restatement of metro_person_steps_labels, metro_person_rays and metro_associate_tracks_rays, written from the header
comment of include/metro_hip.h: the yardstick of tests/test_single_view.py (the kernels' own code compiled for the host) and
tests/test_gpu_single_view.py (the launches).  Nothing in the reference to compare with: one example is one image of one camera.
Deliberately unlike the kernels: the foot of the perpendicular comes from np.linalg.lstsq on d tau ~ w, R from an orthonormal
basis of d's null space (SVD), the persons' steps from Python dicts of labels, the rays from tests/triangulation_ref.py's
vectorised ones; the walk is tests/follow_tracks_ref.py's (its steps, its point cost, its greedy order) and
tests/assign_tracks_ref.py's solver with the ray cost hooked in per row, and the filter step is tests/track_smoothing_ref.py's.
Also the cases both test files run, with the margins that say how far each is from a decision a last bit could flip, and the
stream that shows what the feature is for: a person two of three cameras lose for 1.5 s."""
import functools

import numpy as np

from tests import assign_tracks_ref as AR
from tests import follow_tracks_ref as FT
from tests import track_smoothing_ref as TS
from tests import triangulation_ref as TR

COST_MM = FT.COST_MM            # costs, z and tau: two fp64 evaluations of the same inputs, then one fp32 rounding
POINT_MM = 1e-3
R_REL = TS.COVARIANCE_REL       # R within 1e-6 of its block's largest entry
STATE_REL = FT.STATE_REL
MARGIN_MM = FT.MARGIN_MM
TAU_MARGIN_MM = 1e-1            # every tau a cost or a placement looked at is at least this far from 0
DEPTH_SIGMA = 1000.0
SENTINEL = -7


# ---- metro_person_steps_labels -----------------------------------------------------------------------------------------------

def person_steps_labels(person_index, n_persons, n, box_step, step_times):
    """-> (person_step int32 [n], person_times float64 [n], step_rows int32 [n], step_starts int32 [S + 1], single_box int32 [n])."""
    step_times = np.asarray(step_times, np.float64).reshape(-1)
    n_steps = len(step_times)
    boxes = {}
    for b, p in enumerate(np.asarray(person_index).reshape(-1).tolist()):
        if 0 <= p < min(int(n_persons), n):
            boxes.setdefault(p, []).append(b)
    person_step, single_box = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    for p, own in boxes.items():
        steps = [int(box_step[b]) for b in own if 0 <= int(box_step[b]) < n_steps]
        if steps:
            person_step[p] = min(steps)
            if len(own) == 1:
                single_box[p] = own[0]
    order = sorted((int(s), p) for p, s in enumerate(person_step) if s >= 0)
    step_rows = np.full(n, -1, np.int32)
    step_rows[:len(order)] = [p for _, p in order]
    step_starts = np.asarray([sum(s < k for s, _ in order) for k in range(n_steps + 1)], np.int32)
    person_times = np.array([step_times[s] if s >= 0 else np.nan for s in person_step], np.float64)
    return person_step, person_times, step_rows, step_starts, single_box


def labels_cases():
    """name -> dict(person_index, n_persons, n, box_step, step_times): n = 1, 2, 127, 128; a label out of range; all single; none; 300 boxes."""
    rng = np.random.default_rng(11)
    times = lambda s: np.arange(s) / 32.0 + 5.0
    cases = {
        'n1-single': dict(person_index=[0], n_persons=1, n=1, box_step=[0], step_times=times(1)),
        'n2-pair': dict(person_index=[0, 0], n_persons=1, n=2, box_step=[1, 1], step_times=times(2)),
        'n2-singles': dict(person_index=[0, 1], n_persons=2, n=2, box_step=[1, 0], step_times=times(2)),
        'label-out-of-range': dict(person_index=[0, 7, -3, 1, 0, 2], n_persons=3, n=6, box_step=[1, 0, 0, 2, 1, 0], step_times=times(3)),
        'count-below-labels': dict(person_index=[0, 1, 2, 3], n_persons=2, n=4, box_step=[0, 1, 0, 1], step_times=times(2)),
        'step-out-of-range': dict(person_index=[0, 0, 1, 2, 2], n_persons=3, n=5, box_step=[5, 1, -1, 0, 9], step_times=times(2)),
        'count-0': dict(person_index=[0, 1, 2], n_persons=0, n=3, box_step=[0, 0, 0], step_times=times(1)),
    }
    for n in (127, 128):
        labels = np.repeat(np.arange(n), 2)[:n]             # pairs 0 0 1 1 ...: nobody single (the last of an odd n is)
        steps = rng.integers(0, 3, n)[labels]
        cases[f'n{n}-pairs'] = dict(person_index=labels, n_persons=int(labels.max()) + 1, n=n, box_step=steps, step_times=times(3))
        cases[f'n{n}-all-single'] = dict(person_index=rng.permutation(n), n_persons=n, n=n, box_step=rng.integers(0, 65, n),
                                         step_times=times(65))
        mixed = np.concatenate([np.repeat(np.arange(n // 4), 3), n // 4 + np.arange(n - 3 * (n // 4))])
        cases[f'n{n}-mixed'] = dict(person_index=mixed, n_persons=int(mixed.max()) + 1, n=n, box_step=rng.integers(0, 2, n)[mixed],
                                    step_times=times(2))
    # more boxes than the kernel's chunk of 128: labels of 140 persons on 300 boxes, of which n = 128 and a count of 100 are read
    cases['boxes300'] = dict(person_index=rng.integers(-2, 140, 300), n_persons=100, n=128, box_step=rng.integers(-1, 4, 300),
                             step_times=times(3))
    for c in cases.values():
        c['person_index'], c['box_step'] = np.asarray(c['person_index'], np.int32), np.asarray(c['box_step'], np.int32)
    return cases


# ---- metro_person_rays -----------------------------------------------------------------------------------------------------------

def person_rays(c, spec):
    """c: dict(coords01, cov01, places, weights, n_views, single_box) -> rays float64 [n, Jout, 8]."""
    sk, q = spec.skeleton, c['places']
    d, o, head, ok = TR.rays(c['coords01'], q.inv_intrinsics, q.rot_to_world, q.cam_loc, sk.permutation, sk.out_mirror, spec)
    nv, single = c['n_views'], np.asarray(c['single_box']).reshape(-1)
    n = len(single)
    weighted = c['weights'] == 'covariance'
    if weighted:
        lrc, _ = TR.pixel_scale(spec)
        scale = lrc ** 2 * np.asarray(q.inv_intrinsics, np.float32).astype(np.float64).reshape(-1, 3, 3)[:, 0, 0] ** 2
        cov = np.asarray(c['cov01'], np.float32).astype(np.float64)
        s2 = 0.5 * (np.take_along_axis(cov[..., 0], head, axis=1) + np.take_along_axis(cov[..., 1], head, axis=1)) * scale[:, None]
        s2 = np.where(s2 < 1e-12 * scale[:, None], 1e-12 * scale[:, None], s2)
    out = np.full((n, sk.n_out, 8), np.nan)
    for p, b in enumerate(single.tolist()):
        if not 0 <= b < n:
            continue
        for r in range(sk.n_out):
            use = [b * nv + v for v in range(nv) if ok[b * nv + v, r]]
            w = {i: 1.0 for i in use}
            if weighted:
                with np.errstate(divide='ignore', invalid='ignore'):
                    w = {i: 1.0 / s2[i, r] for i in use}
                use = [i for i in use if np.isfinite(w[i]) and w[i] > 0]
            if not use:
                continue
            total = np.sum([w[i] * d[i, r] for i in use], axis=0)
            length = np.linalg.norm(total)
            if not (np.isfinite(length) and length > 0):
                continue
            out[p, r] = np.concatenate([o[use[0]], total / length, [1.0 / sum(w[i] for i in use) if weighted else 0.0], [len(use)]])
    return out


def compare_rays(got, want):
    """NaN pattern and the view count exactly; o exactly (fp32 values); d within 1e-12; sigma2 within 1e-12 relative."""
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), 'NaN pattern of the rays'
    have = ~np.isnan(want[..., 0])
    if not have.any():
        return 0.0
    g, w = got[have], want[have]
    assert np.array_equal(g[:, :3], w[:, :3]) and np.array_equal(g[:, 7], w[:, 7])
    worst = float(np.abs(g[:, 3:6] - w[:, 3:6]).max())
    assert worst <= 1e-12, worst
    assert (np.abs(g[:, 6] - w[:, 6]) <= 1e-12 * np.abs(w[:, 6])).all()
    return worst


# ---- the ray as a measurement ------------------------------------------------------------------------------------------------------

def foot(p_hat, o, d):
    """-> (tau, distance of p_hat from the line): tau solves d tau ~ p_hat - o in the least-squares sense."""
    w = np.asarray(p_hat, np.float64) - o
    tau = float(np.linalg.lstsq(np.asarray(d, np.float64).reshape(3, 1), w, rcond=None)[0][0])
    return tau, float(np.linalg.norm(w - tau * d))


def ray_noise(d, sigma2, tau, depth_sigma):
    """R: sigma2 tau^2 on the two directions of an orthonormal basis of d's null space, depth_sigma^2 on d."""
    basis = np.linalg.svd(np.asarray(d, np.float64).reshape(1, 3))[2][1:]
    return sigma2 * tau * tau * (basis.T @ basis) + depth_sigma ** 2 * np.outer(d, d)


def _predicted(ws_joint, t):
    dt = max(t - ws_joint[27], 0.0)
    return ws_joint[:3] + dt * ws_joint[3:6]


def ray_cost(ws_slot, ray, t, c):
    """-> (cost fp32, the smallest |tau| looked at)."""
    tl = ws_slot[:, 27]
    have = ~np.isnan(tl)
    if not have.any():
        return np.float32(np.inf), np.inf
    ok = have & np.isfinite(ray[:, :7]).all(axis=1)
    if ok.sum() < c['min_joints'] or ok.sum() < 1 or tl[have].max() < t - c['max_age']:
        return np.float32(np.inf), np.inf
    dists, taus = [], []
    for j in np.flatnonzero(ok):
        tau, dist = foot(_predicted(ws_slot[j], t), ray[j, :3], ray[j, 3:6])
        taus.append(abs(tau))
        dists.append(c['clip'] if not tau > 0 else min(dist, c['clip']))
    return np.float32(np.sqrt(np.mean(np.square(dists)))), min(taus)


def associate(c, assignment='greedy', placed=None):
    """One launch on the case's table -> follow_tracks_ref.associate's dict plus poses / cov (the fp32 arrays with the placed
    joints written), ray_depth, n_unplaced, margin_tau and, per rule, margin_pick or margin_opt / margin_needed.
    placed = (poses, cov): the filter reads THESE fp32 arrays (the kernel's own z and R) instead of the ones placed here, so
    that the states compare at fp64 precision; the arrays returned are still this function's own."""
    poses = np.array(c['poses'], np.float32)
    n, nj = poses.shape[:2]
    cov = np.array(c['cov'], np.float32).reshape(n, nj, 9)
    times = np.asarray(c['times'], np.float64)
    single, rays, depth_sigma = np.asarray(c['single_box']).reshape(-1), np.asarray(c['rays'], np.float64), float(c['depth_sigma'])
    state, ids = np.array(c['state'], np.float64), np.array(c['ids'], np.int32)
    next_id = int(np.asarray(c['next_id']).reshape(-1)[0])
    cap = len(ids)
    steps = FT._steps(c)
    ws = state.copy()
    tracks = {}
    t_first = times[steps[0][0][1]] if steps else None
    for slot in range(cap):
        tl = ws[slot, :, 27]
        live = not np.isnan(tl).all()
        if live and t_first is not None and np.nanmax(tl) < t_first - c['max_age']:
            state[slot, :, 27] = ws[slot, :, 27] = np.nan
            live = False
        if live:
            tracks[slot] = {'id': int(ids[slot]), 'rows': []}
    track_index, track_id = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    cost_out = np.full(n, np.nan, np.float32)
    ray_depth = np.full((n, nj), np.nan, np.float32)
    n_new = n_dropped = n_unplaced = n_pairs = 0
    margin_pick = margin_gate = margin_opt = margin_tau = np.inf
    needed, total = MARGIN_MM, 0.0
    g = np.float32(c['max_cost'])
    for listed in steps:
        t = times[listed[0][1]]
        slots = sorted(tracks)
        cm = np.full((len(listed), len(slots)), np.inf, np.float32)
        for bi, (k, row) in enumerate(listed):
            for si, slot in enumerate(slots):
                if single[row] >= 0:
                    cm[bi, si], near = ray_cost(ws[slot], rays[row], t, c)
                    margin_tau = min(margin_tau, near)
                else:
                    cm[bi, si] = FT._cost(ws[slot], poses[row].astype(np.float64), t, c)
        finite = cm[np.isfinite(cm)].astype(np.float64)
        if len(finite):
            margin_gate = min(margin_gate, float(np.abs(finite - c['max_cost']).min()))
        assigned = {}
        if len(slots) and assignment == 'optimal':
            step_total, pairs, margin = AR.solve(np.where(cm < g, cm.astype(np.float64) - np.float64(g), np.inf))
            margin_opt, needed = min(margin_opt, margin), max(needed, AR.margin_needed(len(slots), len(listed)))
            total += step_total
            assigned = {listed[bi][0]: (slots[si], cm[bi, si]) for bi, si in pairs.items()}
        elif len(slots):
            order = sorted(((cm[bi, si], slots[si], listed[bi][0]) for bi in range(len(listed)) for si in range(len(slots))
                            if np.isfinite(cm[bi, si])), key=lambda e: (e[0], e[1], e[2]))
            taken_slots, taken_boxes = set(), set()
            for v, slot, k in order:
                if v < g and slot not in taken_slots and k not in taken_boxes:
                    taken_slots.add(slot), taken_boxes.add(k)
                    assigned[k] = (slot, v)
                    others = [float(w) for w, s2, k2 in order if (s2 == slot) != (k2 == k)]
                    if others:
                        margin_pick = min(margin_pick, min(abs(w - float(v)) for w in others))
        n_pairs += len(assigned)
        for k, row in listed:
            if k in assigned:
                slot, v = assigned[k]
                cost_out[row] = v
            elif single[row] >= 0:
                n_unplaced += 1                            # a ray row is never born
                continue
            else:
                free = [s for s in range(cap) if s not in tracks]
                if not free or not np.isfinite(poses[row]).all(axis=1).any():
                    n_dropped += 1
                    continue
                slot = free[0]
                tracks[slot] = {'id': next_id, 'rows': []}
                next_id += 1
                n_new += 1
            tracks[slot]['rows'].append(row)
            track_index[row], track_id[row] = slot, tracks[slot]['id']
            if single[row] >= 0:
                for j in range(nj):
                    if np.isnan(ws[slot, j, 27]) or not np.isfinite(rays[row, j, :7]).all():
                        continue
                    o, d = rays[row, j, :3], rays[row, j, 3:6]
                    tau, _ = foot(_predicted(ws[slot, j], t), o, d)
                    margin_tau = min(margin_tau, abs(tau))
                    if not tau > 0:
                        continue
                    poses[row, j] = (o + tau * d).astype(np.float32)
                    cov[row, j] = ray_noise(d, rays[row, j, 6], tau, depth_sigma).reshape(9).astype(np.float32)
                    ray_depth[row, j] = np.float32(tau)
            src = (poses, cov) if placed is None else placed
            ws[slot] = TS.smooth_tracks(src[0], src[1], times, [row], [0, 1], 'filter', 'covariance', c['q'], c['r_floor'],
                                        c['cov_scale'], c['v0'], c['gate'], ws[slot][None])[4][0]
    ids_out = np.full(cap, -1, np.int32)
    rows, starts = [], [0]
    for slot in range(cap):
        if slot in tracks:
            ids_out[slot] = tracks[slot]['id']
            rows += tracks[slot]['rows']
        starts.append(len(rows))
    rows_out = np.full(n, -1, np.int32)
    rows_out[:len(rows)] = rows
    return dict(track_index=track_index, track_id=track_id, cost=cost_out, rows=rows_out, starts=np.asarray(starts, np.int32),
                n_new=n_new, n_dropped=n_dropped, n_unplaced=n_unplaced, state=state, ids=ids_out, next_id=next_id, working=ws,
                poses=poses, cov=cov, ray_depth=ray_depth, margin_pick=margin_pick, margin_gate=margin_gate, margin_opt=margin_opt,
                margin_needed=needed, margin_tau=margin_tau, total=total, n_pairs=n_pairs)


def check_margins(want, assignment):
    """Every decision at least 1e-2 mm from flipping (the optimal rule: its own bound), every tau 1e-1 mm from 0."""
    assert want['margin_gate'] >= MARGIN_MM, want['margin_gate']
    assert want['margin_tau'] >= TAU_MARGIN_MM, want['margin_tau']
    if assignment == 'optimal':
        assert want['margin_opt'] >= want['margin_needed'], (want['margin_opt'], want['margin_needed'])
    else:
        assert want['margin_pick'] >= MARGIN_MM, want['margin_pick']


def compare(got, want, c):
    """follow_tracks_ref.compare on what the walk shares with it; n_unplaced and the NaN patterns of z, R and tau exactly; z and
    tau within 1e-3 mm; R within 1e-6 of its block's largest entry; a point row's pose and covariance untouched.
    -> (worst cost mm, worst state rel, worst z mm, worst tau mm, worst R rel)."""
    worst_cost, worst_state = FT.compare(got, want, c)
    assert int(np.asarray(got['n_unplaced']).reshape(-1)[0]) == want['n_unplaced']
    n, nj = want['poses'].shape[:2]
    gp, gc, gd = np.asarray(got['poses']).reshape(n, nj, 3), np.asarray(got['cov']).reshape(n, nj, 9), np.asarray(got['ray_depth']).reshape(n, nj)
    point = np.asarray(c['single_box']).reshape(-1) < 0
    assert np.array_equal(gp[point], np.asarray(c['poses'], np.float32)[point], equal_nan=True)
    assert np.array_equal(gc[point], np.asarray(c['cov'], np.float32).reshape(n, nj, 9)[point], equal_nan=True)
    for g, w, name in ((gp, want['poses'], 'z'), (gc, want['cov'], 'R'), (gd, want['ray_depth'], 'tau')):
        assert np.array_equal(np.isnan(g), np.isnan(w)), f'NaN pattern of {name}'
    placed = ~np.isnan(want['ray_depth'])
    assert not placed[point].any()
    if not placed.any():
        return worst_cost, worst_state, 0.0, 0.0, 0.0
    worst_z = float(np.abs(gp[placed].astype(np.float64) - want['poses'][placed]).max())
    worst_tau = float(np.abs(gd[placed].astype(np.float64) - want['ray_depth'][placed]).max())
    scale = np.abs(want['cov'][placed]).max(axis=1, keepdims=True).astype(np.float64)
    worst_r = float((np.abs(gc[placed].astype(np.float64) - want['cov'][placed]) / scale).max())
    assert worst_z <= POINT_MM and worst_tau <= POINT_MM and worst_r <= R_REL, (worst_z, worst_tau, worst_r)
    return worst_cost, worst_state, worst_z, worst_tau, worst_r


# ---- cases: scenes of follow_tracks_ref / assign_tracks_ref in which some rows are seen by one camera ---------------------------

CAMERA = np.array([400.0, -250.0, -2500.0])                 # every scene stands about z = 3000: all of it in front, tau about 5.5 m


def to_rays(c, rows, origin=CAMERA, seed=0, joints=None, depth_sigma=DEPTH_SIGMA):
    """The rows `rows` of the case become ray rows: the ray of every joint (or of `joints`) runs from `origin` through the row's
    pose, with a lateral variance of (0.8 to 2 mm at 1 m)^2; pose and covariance become NaN, as the triangulation leaves them.
    Every other row keeps NaN rays.  The case is always in covariance mode."""
    rng = np.random.default_rng(1000 + seed)
    n, nj = c['poses'].shape[:2]
    c = dict(c, poses=np.array(c['poses'], np.float32), measurement='covariance', depth_sigma=depth_sigma)
    c['cov'] = np.array(TS._random_cov(rng, (n, nj), sigma=(1.0, 4.0)) if c['cov'] is None else c['cov'], np.float32).reshape(n, nj, 9)
    if 'single_box' not in c:
        c['single_box'], c['rays'] = np.full(n, -1, np.int32), np.full((n, nj, 8), np.nan)
    else:
        c['single_box'], c['rays'] = c['single_box'].copy(), c['rays'].copy()
    for row in rows:
        p = c['poses'][row].astype(np.float64)
        which = np.arange(nj) if joints is None else np.asarray(joints)
        d = p[which] - origin
        c['rays'][row, which, :3] = np.asarray(origin, np.float32).astype(np.float64)
        c['rays'][row, which, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
        c['rays'][row, which, 6] = rng.uniform(0.8e-3, 2e-3, len(which)) ** 2
        c['rays'][row, which, 7] = 1.0
        c['single_box'][row] = row
        c['poses'][row], c['cov'][row] = np.nan, np.nan
    return c


def _rows_at(c, frames, persons=None, fps=32.0):
    keep = np.isin(np.round(c['times'] * fps).astype(int), list(frames)) & (c['person'] >= 0)
    if persons is not None:
        keep &= np.isin(c['person'], list(persons))
    return np.flatnonzero(keep)


def shape_case(n_persons, n_frames, nj, capacity, seed, ray_frames, ray_persons=None):
    """follow_tracks_ref.shape_case (persons on a 1 m grid) with the rows of `ray_persons` (None: all) at `ray_frames` as rays."""
    c = FT.shape_case(n_persons, n_frames, nj, capacity, seed)
    return to_rays(c, _rows_at(c, ray_frames, ray_persons), seed=seed)


def case_competing(ray_x, point_x):
    """One slot at x = 0; a ray row whose person stands at ray_x and a point row at point_x want it (all share one joint cloud,
    so the point cost is |point_x| and the ray cost nearly |ray_x|: the camera looks almost along z).  The loser: the point row
    is born, the ray row is unplaced."""
    c = AR.table_case([0.0], [[point_x, ray_x]], capacity=3, seed=91)
    return to_rays(c, [1], seed=91)


def case_partial():
    """Slot 0 holds a state on joints 0-11 only, the ray row has rays on joints 2-16 only: ten joints cost, ten are placed, the
    joints 12-16 of the slot stay without a state (no depth to start one from), joints 0-1 are bridged."""
    c = AR.table_case([0.0, 1500.0], [[30.0, 1480.0]], capacity=3, seed=92, slot_joints={0: range(12)})
    return to_rays(c, [0], seed=92, joints=range(2, 17))


def case_exhausted():
    """Three persons, two slots, four frames (follow_tracks_ref's): the third person is dropped at every step -- and unplaced, not
    dropped, at frame 2, where one camera sees it; person 0 is a ray row at frame 3."""
    c = FT.case_exhausted()
    return to_rays(c, list(_rows_at(c, [2], [2])) + list(_rows_at(c, [3], [0])), seed=93)


def case_first_sight():
    """A person one camera sees before any track exists is never born: unplaced at frames 0 and 1, born at frame 2 as a point."""
    c = FT.shape_case(2, 4, 17, 4, 94)
    return to_rays(c, _rows_at(c, [0, 1], [1]), seed=94)


CASES = {
    # T = 1, 2, 65, 128; steps of 1, 64, 65, 128 boxes; J = 1, 17, 64
    'T1-m1-ray-only-step': lambda: shape_case(1, 3, 17, 1, 101, [2]),
    'T2-m2': lambda: shape_case(2, 4, 17, 2, 102, [2, 3], [0]),
    'T65-m64': lambda: shape_case(64, 3, 17, 65, 103, [1, 2], range(0, 64, 4)),
    'T65-m65-j1': lambda: shape_case(65, 3, 1, 65, 104, [2], range(0, 65, 3)),
    'T128-m128-j1-full-table': lambda: shape_case(128, 3, 1, 128, 105, [1, 2], range(1, 128, 4)),
    'j64': lambda: shape_case(3, 4, 64, 4, 106, [2, 3], [1, 2]),
    'all-rays-step': lambda: shape_case(5, 4, 17, 8, 107, [2]),
    'ray-wins': lambda: case_competing(25.0, 40.0),
    'point-wins': lambda: case_competing(45.0, 20.0),
    'partial': case_partial,
    'exhausted': case_exhausted,
    'first-sight': case_first_sight,
}


@functools.lru_cache(maxsize=None)
def case(name):
    """The case, built once and shared by the tests of a session: treat it as read-only."""
    return CASES[name]()


# ---- what the feature is for: two of three cameras lose a person for 1.5 s ------------------------------------------------------

STREAM_FPS = 30.0
STREAM_GAP = (30, 75)            # steps [30, 75): 45 steps = 1.5 s, beyond max_age_s = 1
STREAM_STEPS = 105
STREAM_SWAY_MM = 250.0
STREAM_RAY_NOISE = 1e-4              # rad: a tenth of a pixel at a focal length of 1000 px, 0.8 mm across the ray at 8 m
STREAM_CAMERA = np.array([0.0, -8000.0, 1000.0])            # the camera that keeps seeing the person


def stream_truth(nj=5):
    """One person walking away from the seeing camera at 0.6 m/s while swaying across its view, x = 250 cos(2 (t - 1)) mm: up to
    1 m/s^2 across the ray, which no constant-velocity bridge follows, and a steady speed along it -- the depth stays the
    motion model's under 'rays' too, so a person who turns IN DEPTH while one camera sees them drifts there as before.  The gap
    begins at t = 1 s, where the sway turns: the bridge's error across the ray then grows monotonically for 1.5 s.  Joints: a
    fixed cloud about the centre; joint 0 is the root, at the centre.  -> truth [S, nj, 3] mm."""
    rng = np.random.default_rng(7)
    cloud = np.concatenate([np.zeros((1, 3)), rng.uniform(-300, 300, (nj - 1, 3))])
    t = np.arange(STREAM_STEPS) / STREAM_FPS
    centre = np.stack([STREAM_SWAY_MM * np.cos(2.0 * (t - 1.0)), 600.0 * t, np.full_like(t, 1000.0)], axis=1)
    return centre[:, None, :] + cloud[None]


@functools.lru_cache(maxsize=None)
def stream_case(single_view, nj=5):
    """The stream as one case of the walk, every keyword at its default: one row per step.  Outside the gap the row is a
    triangulated point (0.5 mm of noise per axis, covariance to match); inside, with 'rays', the seeing camera's ray through the
    joint (STREAM_RAY_NOISE of noise, sigma2 to match) and with 'skip' nothing: the person has no step.
    What the scene does NOT show: the depth along the ray is the motion model's, and noisy bearings pull it towards the camera
    (the range bias of every bearing-only EKF).  At 0.1 mrad the root is about 0.15 m short after the 1.5 s; at 0.3 mrad about
    0.4 m, more than max_cost_mm = 300, and the person returns under a new id as under 'skip'."""
    rng = np.random.default_rng(8)
    truth = stream_truth(nj)
    poses = (truth + 0.5 * rng.normal(size=truth.shape)).astype(np.float32)
    cov = np.tile(0.25 * np.eye(3, dtype=np.float32).reshape(9), (STREAM_STEPS, nj, 1))
    times = np.arange(STREAM_STEPS) / STREAM_FPS
    gap = np.arange(*STREAM_GAP)
    listed = np.arange(STREAM_STEPS) if single_view == 'rays' else np.setdiff1d(np.arange(STREAM_STEPS), gap)
    state, ids, next_id = FT.new_table(4, nj)
    c = dict(FT.DEFAULTS, poses=poses, cov=cov, times=times, step_rows=listed.astype(np.int32),
             step_starts=np.arange(len(listed) + 1, dtype=np.int32), state=state, ids=ids, next_id=next_id, min_joints=(nj + 1) // 2,
             person=np.zeros(STREAM_STEPS, int), tie=False, depth_sigma=DEPTH_SIGMA,
             single_box=np.full(STREAM_STEPS, -1, np.int32), rays=np.full((STREAM_STEPS, nj, 8), np.nan))
    if single_view == 'rays':
        for row in gap:
            d = truth[row] - STREAM_CAMERA
            d = d / np.linalg.norm(d, axis=1, keepdims=True) + rng.normal(size=d.shape) * STREAM_RAY_NOISE
            c['rays'][row, :, :3] = STREAM_CAMERA
            c['rays'][row, :, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
            c['rays'][row, :, 6] = STREAM_RAY_NOISE ** 2
            c['rays'][row, :, 7] = 1.0
            c['single_box'][row] = row
            c['poses'][row], c['cov'][row] = np.nan, np.nan
    return c


def in_calls(run, c, steps_per_call):
    """The case's steps in calls of `steps_per_call`, the table carried -> (track_id [n], {id: state of its slot}, the sums of
    n_new and n_unplaced, the working state after every call)."""
    state, ids, next_id = np.array(c['state']), np.array(c['ids']), np.array(c['next_id'])
    starts, track_id = np.asarray(c['step_starts']), np.full(len(c['poses']), -1, np.int32)
    n_new = n_unplaced = 0
    after = []
    for s in range(0, len(starts) - 1, steps_per_call):
        e = min(s + steps_per_call, len(starts) - 1)
        part = dict(c, step_rows=c['step_rows'][starts[s]:starts[e]], step_starts=starts[s:e + 1] - starts[s], state=state, ids=ids,
                    next_id=next_id)
        r = run(part)
        listed = part['step_rows']
        track_id[listed] = np.asarray(r['track_id'])[listed]
        state, ids, next_id = np.array(r['working']), np.array(r['ids']), np.asarray([r['next_id']], np.int32).reshape(1)
        n_new += int(np.asarray(r['n_new']).reshape(-1)[0])
        n_unplaced += int(np.asarray(r['n_unplaced']).reshape(-1)[0])
        after.append(state)
    return track_id, {int(i): state[slot] for slot, i in enumerate(ids) if i >= 0}, n_new, n_unplaced, after


def across(err, truth_point, camera):
    """The length of `err` across the ray from `camera` to `truth_point`."""
    d = (truth_point - camera) / np.linalg.norm(truth_point - camera)
    return float(np.linalg.norm(err - d * (d @ err)))


# ---- cases of the rays launch: P persons x J joints x V views, at the block boundary of 64 threads ------------------------------

class RaySpec:
    """A spec of J output joints for the rays launch alone: the head holds J + 1 joints, the permutation reverses them, joint r
    mirrors to J - 1 - r.  Duck-types what tests/triangulation_ref.py reads of a ModelSpec."""

    def __init__(self, n_out):
        import types
        self.proc_side, self.stride, self.centered_stride = 256, 32, True
        self.skeleton = types.SimpleNamespace(n_out=n_out, n_head=n_out + 1, permutation=list(range(n_out, 0, -1)),
                                              out_mirror=list(range(n_out - 1, -1, -1)))

    def to_c(self, precision):
        from metro_pose3d_amd import ModelSpec
        cs = ModelSpec(50, self.stride, 'h36m').to_c(precision)
        cs.n_joints_head, cs.n_joints_out = self.skeleton.n_head, self.skeleton.n_out
        for i, p in enumerate(self.skeleton.permutation):
            cs.permutation[i] = p
        return cs


def rays_case(n_persons, n_out, n_views, seed, weights):
    """Every box a camera of its own about 5 m from the origin, its views rolled about the optical axis and every second one
    flipped (det rot_to_world < 0), joints anywhere in the crop.  single_box: most persons their own box, one in five none, one
    an index past the boxes; one view in seven has a NaN joint, one in nine a NaN variance, one box a zero variance (floored)."""
    from metro_pose3d_amd import frames as FR
    rng = np.random.default_rng(seed)
    spec = RaySpec(n_out)
    m = n_persons * n_views
    rot, loc, inv_k = np.zeros((m, 3, 3), np.float32), np.zeros((m, 3), np.float32), np.zeros((m, 3, 3), np.float32)
    for b in range(n_persons):
        centre = rng.normal(size=3)
        centre = 5000.0 * centre / np.linalg.norm(centre)
        z = -centre / np.linalg.norm(centre)
        for v in range(n_views):
            x = np.cross(z, rng.normal(size=3))
            x /= np.linalg.norm(x)
            r = np.stack([x, np.cross(z, x), z], axis=1)
            if v % 2:
                r[:, 0] = -r[:, 0]
            f = rng.uniform(200.0, 400.0)
            rot[b * n_views + v], loc[b * n_views + v] = r, centre
            inv_k[b * n_views + v] = [[1 / f, 0, -128 / f], [0, 1 / f, -128 / f], [0, 0, 1]]
    eye = np.tile(np.eye(3, dtype=np.float32), (m, 1, 1))
    places = FR.PlacementParams(np.zeros(m, np.int32), inv_k, eye.copy(), rot, loc, eye.copy(), eye.copy(), np.zeros((m, 5), np.float32))
    coords01 = rng.uniform(0.05, 0.95, (m, n_out + 1, 3)).astype(np.float32)
    cov01 = TR.cov01_for(rng.uniform(0.2, 3.0, (m, n_out + 1)), spec, (m, n_out + 1))
    flat = np.arange(m * (n_out + 1))
    coords01.reshape(-1, 3)[flat[3::7], 0] = np.nan
    cov01.reshape(-1, 6)[flat[5::9], 1] = np.nan
    cov01[0, :, :2] = 0.0
    single = np.arange(n_persons, dtype=np.int32)
    single[2::5] = -1
    if n_persons > 3:
        single[3] = n_persons + 3
    return dict(coords01=coords01, cov01=cov01, places=places, weights=weights, n_views=n_views, single_box=single, spec=spec)


RAY_CASES = {f'P{p}-J{j}-V{v}-{w}': (p, j, v, 200 + i, w) for i, (p, j, v, w) in enumerate((
    (1, 1, 1, 'covariance'), (9, 7, 2, 'covariance'), (64, 1, 1, 'uniform'), (8, 8, 3, 'covariance'), (65, 1, 2, 'covariance'),
    (13, 5, 3, 'uniform'), (4, 17, 2, 'covariance')))}           # P J = 1, 63, 64, 64, 65, 65, 68; V = 1, 2, 3


@functools.lru_cache(maxsize=None)
def rays_case_and_expected(name):
    c = rays_case(*RAY_CASES[name])
    return c, person_rays(c, c['spec'])
