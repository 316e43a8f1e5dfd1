"""fp64 NumPy restatement of metro_associate_tracks, written from the header comment of include/metro_hip.h: the yardstick of
tests/test_follow_tracks.py (the kernel's steps compiled for the host) and tests/test_gpu_follow_tracks.py (the launch).
Nothing in the reference to compare with: one example is one image.  Deliberately unlike the kernel: the tracks are Python
dicts keyed by slot, the assignment sorts all candidate pairs once instead of striking rows and columns of a matrix, the
distances are vectorised over the joints, and the filter step is tests/track_smoothing_ref.py's (dense matrices, np.linalg)
run on one-row groups.  Costs are rounded to fp32 where the kernel rounds them.  Also the test cases both files run, and the
decision margin that says how far each case is from a decision a last-bit difference could flip."""
import functools

import numpy as np

from tests import track_smoothing_ref as TS

COST_MM = 1e-3            # kernel vs this file: both fp64 on identical fp32 inputs, then one fp32 rounding (<= 3.1e-5 below 600 mm)
STATE_REL = 1e-9          # x and P of the working state: cofactors there, LAPACK here (tests/test_track_smoothing.py's bound)
MARGIN_MM = 1e-2          # every non-tie case keeps its decisions at least this far from flipping
SENTINEL = -7
DEFAULTS = dict(measurement='covariance', q=4e6, r_floor=1.0, cov_scale=1.0, v0=2000.0, gate=0.0, max_cost=300.0, clip=600.0,
                max_age=1.0)


def new_table(capacity, nj):
    state = np.zeros((capacity, nj, 28))
    state[..., 27] = np.nan
    return state, np.full(capacity, -1, np.int32), np.zeros(1, np.int32)


def _steps(c):
    """[(positions, rows)] per step as the header reads the CSR: starts clamped, at most 128 positions, rows outside skipped."""
    n, rows, starts = len(c['poses']), np.asarray(c['step_rows']), np.asarray(c['step_starts'])
    out = []
    for s in range(len(starts) - 1):
        lo, hi = max(int(starts[s]), 0), min(int(starts[s + 1]), len(rows))
        listed = [(k, int(rows[lo + k])) for k in range(min(max(hi - lo, 0), 128)) if 0 <= int(rows[lo + k]) < n]
        if listed:
            out.append(listed)
    return out


def _cost(ws_slot, z, t, c, use_velocity=True):
    tl = ws_slot[:, 27]
    have = ~np.isnan(tl)
    if not have.any():
        return np.float32(np.inf)
    ok = have & np.isfinite(z).all(axis=1)
    if ok.sum() < c['min_joints'] or tl[have].max() < t - c['max_age']:
        return np.float32(np.inf)
    dt = np.maximum(t - tl[ok], 0.0)
    pred = ws_slot[ok, :3] + (dt[:, None] * ws_slot[ok, 3:6] if use_velocity else 0.0)
    d = np.minimum(np.linalg.norm(z[ok] - pred, axis=1), c['clip'])
    return np.float32(np.sqrt(np.mean(d ** 2)))


def associate(c, use_velocity=True):
    """One launch on the case's table -> dict of everything the launch writes (the table's new state / ids / next_id included),
    `working` the working state, and the decision margins `margin_pick` and `margin_gate` in mm.  use_velocity=False drops
    dt v from the prediction (a cost on the last filtered position), for experiments."""
    poses = np.asarray(c['poses'], np.float32)
    n, nj = poses.shape[:2]
    times = np.asarray(c['times'], np.float64)
    state, ids = np.array(c['state'], np.float64), np.array(c['ids'], np.int32)
    next_id = int(np.asarray(c['next_id']).reshape(-1)[0])
    cap = len(ids)
    steps = _steps(c)
    ws = state.copy()
    tracks = {}                                                   # slot -> {'id', 'rows'}: the slots that hold a track
    t_first = times[steps[0][0][1]] if steps else None
    for slot in range(cap):
        tl = ws[slot, :, 27]
        live = not np.isnan(tl).all()
        if live and t_first is not None and np.nanmax(tl) < t_first - c['max_age']:
            state[slot, :, 27] = ws[slot, :, 27] = np.nan         # retired
            live = False
        if live:
            tracks[slot] = {'id': int(ids[slot]), 'rows': []}
    track_index, track_id = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    cost_out = np.full(n, np.nan, np.float32)
    n_new = n_dropped = 0
    margin_pick = margin_gate = np.inf
    for listed in steps:
        t = times[listed[0][1]]
        costs = {(slot, k): _cost(ws[slot], poses[row].astype(np.float64), t, c, use_velocity) for slot in tracks for k, row in listed}
        finite = {p: v for p, v in costs.items() if np.isfinite(v)}
        if finite:
            margin_gate = min(margin_gate, min(abs(float(v) - c['max_cost']) for v in finite.values()))
        taken_slots, taken_boxes, assigned = set(), set(), {}
        for (slot, k), v in sorted(finite.items(), key=lambda kv: (kv[1], kv[0][0], kv[0][1])):
            if v < np.float32(c['max_cost']) and slot not in taken_slots and k not in taken_boxes:
                taken_slots.add(slot), taken_boxes.add(k)
                assigned[k] = (slot, v)
                others = [float(w) for (s2, k2), w in finite.items() if (s2 == slot) != (k2 == k)]
                if others:
                    margin_pick = min(margin_pick, min(abs(w - float(v)) for w in others))
        for k, row in listed:
            if k in assigned:
                slot, v = assigned[k]
                cost_out[row] = v
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
            # the filter step of the smoothing restatement, on a group of this one row
            ws[slot] = TS.smooth_tracks(poses, c['cov'], times, [row], [0, 1], 'filter', c['measurement'], c['q'], c['r_floor'],
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
                n_new=n_new, n_dropped=n_dropped, state=state, ids=ids_out, next_id=next_id, working=ws,
                margin_pick=margin_pick, margin_gate=margin_gate)


# ---- cases -------------------------------------------------------------------------------------------------------------------

def time_steps(times):
    """frames.time_steps without the package: (step_rows, step_starts)."""
    times = np.asarray(times, np.float64)
    order = np.argsort(times, kind='stable')
    new = np.concatenate([[True], times[order][1:] != times[order][:-1]])
    return order.astype(np.int32), np.concatenate([np.flatnonzero(new), [len(times)]]).astype(np.int32)


def scene(centres, nj=17, capacity=8, seed=0, noise=2.0, fps=32.0, shuffle=True, extra_rows=1, **params):
    """centres: {person: {frame: (x, y, z) mm}} -> a case.  Every person is a fixed cloud of nj joints within 300 mm of its centre
    plus `noise` mm of measurement noise per joint; boxes are scrambled in memory (so also within each step), `extra_rows`
    rows are listed in no step; fps = 32 keeps the times exact in binary.  `person` [n] is the truth (-1: in no step)."""
    rng = np.random.default_rng(seed)
    boxes = [(f, p) for p, path in centres.items() for f in path]
    n = len(boxes) + extra_rows
    where = rng.permutation(n) if shuffle else np.arange(n)
    poses = rng.uniform(-100, 100, (n, nj, 3)).astype(np.float32)
    times, person = rng.uniform(50, 60, n), np.full(n, -1)
    cloud = {p: rng.uniform(-300, 300, (nj, 3)) for p in centres}
    for i, (f, p) in enumerate(boxes):
        poses[where[i]] = (np.asarray(centres[p][f], np.float64) + cloud[p] + rng.normal(size=(nj, 3)) * noise).astype(np.float32)
        times[where[i]], person[where[i]] = f / fps, p
    listed = np.sort(where[:len(boxes)])
    step_rows, step_starts = time_steps(times[listed])
    state, ids, next_id = new_table(capacity, nj)
    c = dict(DEFAULTS, poses=poses, cov=TS._random_cov(rng, (n, nj), sigma=(1.0, 4.0)), times=times, step_rows=listed[step_rows].astype(np.int32),
             step_starts=step_starts, state=state, ids=ids, next_id=next_id, min_joints=(nj + 1) // 2, person=person, tie=False)
    c.update(params)
    return c


def _line(p0, v_per_frame, frames):
    return {f: np.asarray(p0, np.float64) + np.asarray(v_per_frame, np.float64) * f for f in frames}


def case_crossing():
    """Two persons of nearly the same build (joint clouds within 30 mm of each other) walking through each other at different
    speeds: their centres coincide at frame 4; at frame 5 person 1's box is the nearer one to where person 0 was last seen."""
    c = scene({0: _line((-600, 0, 3000), (150, 0, 0), range(9)), 1: _line((200, 0, 3000), (-50, 0, 0), range(9))}, seed=21)
    rng = np.random.default_rng(22)
    cloud = rng.uniform(-300, 300, (17, 3))
    clouds = (cloud, cloud + rng.uniform(-30, 30, (17, 3)))
    for i in np.flatnonzero(c['person'] >= 0):
        f = c['times'][i] * 32.0
        centre = np.array([-600 + 150 * f, 0, 3000]) if c['person'][i] == 0 else np.array([200 - 50 * f, 0, 3000])
        c['poses'][i] = (centre + clouds[c['person'][i]] + rng.normal(size=(17, 3)) * 2.0).astype(np.float32)
    return c


def case_absence_within():
    """Person 0 is absent for frames 4-11 (8 frames = 0.25 s < max_age_s) and returns where its velocity says."""
    frames = [f for f in range(16) if not 4 <= f < 12]
    return scene({0: _line((0, 0, 3000), (6, 2, 0), frames), 1: _line((1500, 0, 3500), (-4, 0, 3), range(16))}, seed=23)


def case_absence_beyond():
    """Person 0 is absent for 40 frames (1.25 s > max_age_s): its slot is too old to continue, the person returns under a new id
    in a new slot (no slot is retired inside a call)."""
    frames = [0, 1, 2, 3] + list(range(44, 48))
    return scene({0: _line((0, 0, 3000), (2, 0, 0), frames), 1: _line((1500, 0, 3500), (-1, 0, 1), range(0, 48, 2))}, seed=24)


def case_newcomer():
    return scene({0: _line((0, 0, 3000), (5, 0, 0), range(8)), 1: _line((1200, 300, 3300), (0, 4, 0), range(3, 8))}, seed=25)


def case_two_near_one():
    """At frame 3 a second box appears 120 mm from person 0's track (inside max_cost_mm): the nearer box continues the track,
    the other is born."""
    return scene({0: _line((0, 0, 3000), (4, 0, 0), range(6)), 1: _line((120 + 12, 0, 3000), (4, 0, 0), range(3, 6))}, seed=26, noise=1.0)


def case_exhausted():
    """Three persons, two slots: from frame 0 on the third box of every step is untracked."""
    return scene({p: _line((1000 * p, 0, 3000), (3, 0, 0), range(4)) for p in range(3)}, capacity=2, seed=27, shuffle=False, extra_rows=0)


def case_nan_box():
    """One box of frame 2 has no finite joint (untracked, counted), one of frame 3 has 5 of 17 joints left (fewer than
    min_joints: it cannot continue its track and is born)."""
    c = scene({0: _line((0, 0, 3000), (5, 0, 0), range(5)), 1: _line((1500, 0, 3000), (0, 5, 0), range(5))}, seed=28)
    at = lambda p, f: int(np.flatnonzero((c['person'] == p) & (c['times'] == f / 32.0))[0])
    c['poses'][at(0, 2)] = np.nan
    c['poses'][at(1, 3), 5:] = np.nan
    return c


def case_retired():
    """The table arrives with slot 0 live but last seen 5 s before the call (retired, then reused under a fresh id), slot 1 live
    and recent (continues as id 7), slot 2 free."""
    c = scene({0: _line((0, 0, 3000), (5, 0, 0), range(4)), 1: _line((1500, 0, 3000), (0, 5, 0), range(4))}, capacity=3, seed=29)
    first = {p: int(np.flatnonzero((c['person'] == p) & (c['times'] == 0.0))[0]) for p in (0, 1)}
    for slot, (p, t_last, tid) in enumerate(((0, -5.0, 3), (1, -1 / 32.0, 7))):
        c['state'][slot, :, :3] = c['poses'][first[p]].astype(np.float64)
        c['state'][slot, :, 6 + np.array([0, 6, 11])] = 25.0            # P = diag(25 I, 1e4 I)
        c['state'][slot, :, 6 + np.array([15, 18, 20])] = 1e4
        c['state'][slot, :, 27] = t_last
        c['ids'][slot] = tid
    c['next_id'][0] = 9
    return c


def case_ties():
    """J = 1, isotropic, everything exact in fp32 and dt = 0.  Step 1 (t = 0): slots 0 and 1 wait at x = 0 and x = 128, boxes at
    x = 64 (position 0: costs 64 and 64, the lowest slot takes it) and at x = 192 (position 1: 64 from slot 1 -- after the first
    pick the smallest left).  Slot 2 at x = 1000 with boxes at x = 1000 +- 32 (positions 2, 3): equal costs 32, the lowest
    position wins, the other is born."""
    xs = [64.0, 192.0, 968.0, 1032.0]
    poses = np.zeros((4, 1, 3), np.float32)
    poses[:, 0, 0] = xs
    state, ids, next_id = new_table(4, 1)
    for slot, x in enumerate((0.0, 128.0, 1000.0)):
        state[slot, 0, 0] = x
        state[slot, 0, 6 + np.array([0, 6, 11])] = 4.0
        state[slot, 0, 6 + np.array([15, 18, 20])] = 1e4
        state[slot, 0, 27] = 0.0
        ids[slot] = slot
    next_id[0] = 3
    return dict(DEFAULTS, poses=poses, cov=None, times=np.zeros(4), step_rows=np.arange(4, dtype=np.int32),
                step_starts=np.asarray([0, 4], np.int32), state=state, ids=ids, next_id=next_id, min_joints=1, measurement='isotropic',
                r_floor=2.0, person=np.array([0, 1, 2, 3]), tie=True)


def case_skipped():
    """Row indices outside [0, n) inside a step (skipped, keeping their position), a step holding only such indices, an empty
    step, and offsets beyond [0, n_step_rows] (clamped)."""
    c = scene({0: _line((0, 0, 3000), (5, 0, 0), range(3)), 1: _line((1500, 0, 3000), (0, 5, 0), range(3))}, seed=30)
    n, r, s = len(c['poses']), list(c['step_rows']), list(c['step_starts'])
    rows = r[:2] + [-1, n + 3] + r[2:4] + [n, -2] + r[4:]
    c['step_rows'] = np.asarray(rows, np.int32)
    c['step_starts'] = np.asarray([-3, 3, 3, 6, 8, len(rows) + 5], np.int32)    # {2 boxes, -1}, empty, {n+3, 2 boxes}, bad only, 2 boxes
    assert s == [0, 2, 4, 6]
    return c


def _grid(n_persons, n_frames, seed):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-8, 8, (n_persons, 3))
    return {p: _line((1000.0 * (p % 16), 1000.0 * (p // 16), 3000.0), v[p], range(n_frames)) for p in range(n_persons)}


def shape_case(n_persons, n_frames, nj, capacity, seed, **kw):
    """Persons on a 1 m grid drifting at up to 8 mm a frame: every continuation is far below max_cost_mm, every other pair at clip_mm."""
    return scene(_grid(n_persons, n_frames, seed), nj=nj, capacity=capacity, seed=seed, **kw)


CASES = {
    'crossing': case_crossing, 'absence-within': case_absence_within, 'absence-beyond': case_absence_beyond,
    'newcomer': case_newcomer, 'two-near-one': case_two_near_one, 'exhausted': case_exhausted, 'nan-box': case_nan_box,
    'retired': case_retired, 'ties': case_ties, 'skipped': case_skipped,
    # the loop boundaries of the launch: capacity 1, 2, 65, 128; 1, 64, 65, 128 boxes in a step; J = 1, 17, 64; 1, 2, 65 steps
    'cap1-box1-step1': lambda: shape_case(1, 1, 17, 1, 41),
    'cap1-box2': lambda: shape_case(2, 2, 17, 1, 42),
    'cap2-j1': lambda: shape_case(2, 3, 1, 2, 43, measurement='isotropic', r_floor=3.0),
    'cap65-box64': lambda: shape_case(64, 2, 17, 65, 44),
    'cap65-box65-j1': lambda: shape_case(65, 2, 1, 65, 45),
    'cap128-box128-j1': lambda: shape_case(128, 2, 1, 128, 46),
    'j64': lambda: shape_case(3, 3, 64, 4, 47),
    'steps65': lambda: shape_case(2, 65, 17, 3, 48),
}


@functools.lru_cache(maxsize=None)
def case_and_expected(name):
    """(case, expected) computed once and shared by the tests of a session: treat both as read-only."""
    c = CASES[name]()
    return c, associate(c)


def compare(got, want, c):
    """got: dict with the launch's outputs (track_index, track_id, cost, rows, starts, n_new, n_dropped, ids, next_id, state,
    working).  Integers, NaN patterns and every t_last exactly; costs within COST_MM; x and P of the working state within
    STATE_REL of the slot's largest entry.  -> (worst cost deviation mm, worst relative state deviation)."""
    for k in ('track_index', 'track_id', 'rows', 'starts', 'ids'):
        assert np.array_equal(np.asarray(got[k]).reshape(-1), want[k]), (k, got[k], want[k])
    for k in ('n_new', 'n_dropped', 'next_id'):
        assert int(np.asarray(got[k]).reshape(-1)[0]) == want[k], (k, got[k], want[k])
    g, w = np.asarray(got['cost'], np.float32), want['cost']
    assert np.array_equal(np.isnan(g), np.isnan(w)), 'cost NaN pattern'
    fin = ~np.isnan(w)
    worst_cost = float(np.abs(g[fin].astype(np.float64) - w[fin]).max()) if fin.any() else 0.0
    assert worst_cost <= COST_MM, worst_cost
    assert np.array_equal(got['state'], want['state'], equal_nan=True), 'only the retirement writes the state'
    gw, ww = np.asarray(got['working']), want['working']
    assert np.array_equal(gw[..., 27], ww[..., 27], equal_nan=True), 't_last of the working state'
    live = ~np.isnan(ww[..., 27])
    worst_state = 0.0
    if live.any():
        scale = np.abs(ww[live][:, :27]).max(axis=1, keepdims=True)
        worst_state = float((np.abs(gw[live][:, :27] - ww[live][:, :27]) / scale).max())
    assert worst_state <= STATE_REL, worst_state
    assert np.array_equal(gw[~live][:, :27], np.asarray(c['state'])[~live][:, :27]), 'a joint without a state keeps the copy'
    return worst_cost, worst_state
