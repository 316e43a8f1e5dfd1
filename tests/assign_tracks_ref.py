"""fp64 NumPy restatement of metro_associate_tracks_optimal, written from the header comment of include/metro_hip.h: the
yardstick of tests/test_assign_tracks.py (the kernel's steps compiled for the host) and tests/test_gpu_assign_tracks.py (the
launch).  The walk -- steps, costs, births, filter step, CSR -- is tests/follow_tracks_ref.py's; only the pairing differs, and it
is deliberately unlike the kernel's potentials + Dijkstra:
  * exhaustive search over all partial matchings of admissible pairs when min(live slots, boxes) <= 7 (and the search tree
    has at most EXHAUSTIVE_LEAVES leaves);
  * otherwise successive shortest paths found by Bellman-Ford on the residual graph of the matching, on the gains c - g
    themselves: no dual potentials, no reduced costs, no priority order (`solve_paths`).
scipy is not needed; tests cross-check against scipy.optimize.linear_sum_assignment on the padded matrix where it imports.
Also the cases both test files run, and two decision margins per case:
  margin_gate  every finite cost is at least this far from max_cost (follow_tracks_ref's rule)
  margin_opt   the exact gap between the optimum and the second-best assignment: each pair of the optimum is forbidden in
               turn and the step re-solved; the smallest increase of the total.  (A different assignment either lacks a pair
               of the optimum or adds an admissible pair to it, and the latter can only lower the total.)"""
import functools

import numpy as np

from tests import follow_tracks_ref as FT
from tests import track_smoothing_ref as TS

COST_MM = FT.COST_MM
MARGIN_MM = FT.MARGIN_MM
EXHAUSTIVE_SIDE = 7
EXHAUSTIVE_LEAVES = 200000


def margin_needed(n_slots, n_boxes):
    """The 1e-3 mm allowed per cost cannot change a decision: an assignment has at most min(T, m) pairs, and two differ by at
    most twice that many costs."""
    return max(MARGIN_MM, 2 * min(n_slots, n_boxes) * COST_MM)


# ---- the pairing: w[k][s] = c - g < 0 for an admissible pair, +inf otherwise; minimise the sum over a one-to-one set ----------

def solve_exhaustive(w):
    """-> (total, {box: slot}) by trying every partial matching; None if the tree is too large."""
    nk, ns = w.shape
    if min(nk, ns) > EXHAUSTIVE_SIDE:
        return None
    by_box = nk <= ns
    m = w if by_box else w.T
    options = [np.flatnonzero(np.isfinite(row)).tolist() for row in m]
    if np.prod([len(o) + 1.0 for o in options]) > EXHAUSTIVE_LEAVES:
        return None
    best = [0.0, {}]

    def walk(i, total, taken, pairs):
        if i == len(options):
            if total < best[0]:
                best[0], best[1] = total, dict(pairs)
            return
        walk(i + 1, total, taken, pairs)
        for j in options[i]:
            if j not in taken:
                taken.add(j)
                pairs[i] = j
                walk(i + 1, total + m[i, j], taken, pairs)
                del pairs[i]
                taken.discard(j)
    walk(0, 0.0, set(), {})
    pairs = best[1] if by_box else {j: i for i, j in best[1].items()}
    return best[0], pairs


def _augment(w, k, box_slot, slot_box):
    """One shortest augmenting path from box k in the residual graph of the matching (an edge box -> slot costs w, a matched
    edge back slot -> box costs -w, leaving a box unmatched costs 0), by Bellman-Ford; the matching is changed in place."""
    nk, ns = w.shape
    d_box, d_slot = np.full(nk, np.inf), np.full(ns, np.inf)
    via = np.full(ns, -1)                                          # the box a slot was reached from
    d_box[k] = 0.0
    free = w.copy()
    matched = np.flatnonzero(box_slot >= 0)
    free[matched, box_slot[matched]] = np.inf                      # a matched edge is walked backwards only
    for _ in range(nk + ns + 2):
        cand = d_box[:, None] + free
        src = cand.argmin(axis=0)
        new = cand[src, np.arange(ns)]
        better = new < d_slot
        d_slot[better], via[better] = new[better], src[better]
        changed = bool(better.any())
        for s in np.flatnonzero(slot_box >= 0):
            b = slot_box[s]
            back = d_slot[s] - w[b, s]
            if back < d_box[b]:
                d_box[b], changed = back, True
        if not changed:
            break
    open_slots = np.flatnonzero(slot_box < 0)
    end_slot = open_slots[d_slot[open_slots].argmin()] if len(open_slots) else -1
    end_box = int(d_box.argmin())                                  # this box is left unmatched (box k itself: nothing changes)
    if end_slot >= 0 and d_slot[end_slot] <= d_box[end_box]:
        s = int(end_slot)
    else:
        if end_box == k:
            return
        s = int(box_slot[end_box])
        box_slot[end_box] = -1
        slot_box[s] = -1
    for _ in range(nk + 1):
        b = int(via[s])
        before = int(box_slot[b])
        box_slot[b], slot_box[s] = s, b
        if b == k:
            return
        s = before
    raise AssertionError('the path does not lead back to its box')


def solve_paths(w, start=None, boxes=None):
    """-> (total, {box: slot}); start = (box_slot, slot_box) of a matching that is optimal for its boxes, boxes = those to add."""
    nk, ns = w.shape
    box_slot, slot_box = (np.full(nk, -1), np.full(ns, -1)) if start is None else (start[0].copy(), start[1].copy())
    for k in (range(nk) if boxes is None else boxes):
        _augment(w, k, box_slot, slot_box)
    pairs = {int(b): int(s) for b, s in enumerate(box_slot) if s >= 0}
    return float(sum(w[b, s] for b, s in pairs.items())), pairs


def _reroute(w, box_slot, slot_box, b):
    """The optimum's total rises by this much when its pair (b, s) is forbidden: -w[b, s] plus the shortest way to lead box b's
    unit of flow back to slot s in the residual graph of the optimum without that pair.  The graph has the node "taken out":
    it is entered at 0 from a free slot and from any box (which is then unmatched), and left at 0 into any matched slot (whose
    box has to move on), into a box that is unmatched in the optimum (which may now take a slot) and into s itself (which
    then stays free).  Bellman-Ford again; the optimum has no negative cycle, so the rerouted matching is the optimum of the
    restricted problem."""
    nk, ns = w.shape
    s = box_slot[b]
    d_box, d_slot, d_out = np.full(nk, np.inf), np.full(ns, np.inf), np.inf
    d_box[b] = 0.0
    free = w.copy()
    matched = np.flatnonzero(box_slot >= 0)
    free[matched, box_slot[matched]] = np.inf
    back = matched[matched != b]
    unmatched, open_slots, full_slots = np.flatnonzero(box_slot < 0), np.flatnonzero(slot_box < 0), np.flatnonzero(slot_box >= 0)
    for _ in range(2 * (nk + ns) + 3):
        before = (d_box.copy(), d_slot.copy(), d_out)
        d_slot = np.minimum(d_slot, (d_box[:, None] + free).min(axis=0))
        d_box[back] = np.minimum(d_box[back], d_slot[box_slot[back]] - w[back, box_slot[back]])
        d_out = min(d_out, d_box.min(), d_slot[open_slots].min() if len(open_slots) else np.inf)
        d_box[unmatched] = np.minimum(d_box[unmatched], d_out)
        d_slot[full_slots] = np.minimum(d_slot[full_slots], d_out)
        if np.array_equal(before[0], d_box) and np.array_equal(before[1], d_slot) and before[2] == d_out:
            break
    return float(d_slot[s] - w[b, s])


def solve(w):
    """The optimum of a step -> (total, {box: slot}, margin_opt).  Where both solvers apply they must agree on the total, and
    so must the two ways to the second-best total."""
    small = solve_exhaustive(w)
    total, pairs = solve_paths(w)
    if small is not None:
        assert abs(small[0] - total) <= 1e-9 * max(1.0, abs(total)), (small, total)
        total, pairs = small
    margin = np.inf
    box_slot, slot_box = np.full(w.shape[0], -1), np.full(w.shape[1], -1)
    for b, s in pairs.items():
        box_slot[b], slot_box[s] = s, b
    for b, s in pairs.items():
        rise = _reroute(w, box_slot, slot_box, b)
        if small is not None:
            w2 = w.copy()
            w2[b, s] = np.inf
            again = solve_exhaustive(w2)
            assert abs((again[0] - total) - rise) <= 1e-9 * max(1.0, abs(total)), (again[0] - total, rise)
        margin = min(margin, rise)
    return total, pairs, margin


# ---- the walk ------------------------------------------------------------------------------------------------------------------

def associate(c):
    """One launch of the optimal entry on the case's table -> follow_tracks_ref.associate's dict (without margin_pick) plus
    margin_opt, margin_needed (the bound margin_opt has to keep, from the largest step), total (the sum of c - g over all
    accepted pairs of all steps) and n_pairs."""
    poses = np.asarray(c['poses'], np.float32)
    n, nj = poses.shape[:2]
    times = np.asarray(c['times'], np.float64)
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
    n_new = n_dropped = n_pairs = 0
    margin_opt = margin_gate = np.inf
    needed, total = MARGIN_MM, 0.0
    g = np.float32(c['max_cost'])
    for listed in steps:
        t = times[listed[0][1]]
        slots = sorted(tracks)
        cm = np.full((len(listed), len(slots)), np.inf, np.float32)
        for bi, (k, row) in enumerate(listed):
            for si, slot in enumerate(slots):
                cm[bi, si] = FT._cost(ws[slot], poses[row].astype(np.float64), t, c)
        finite = cm[np.isfinite(cm)].astype(np.float64)
        if len(finite):
            margin_gate = min(margin_gate, float(np.abs(finite - c['max_cost']).min()))
        assigned = {}
        if len(slots):
            w = np.where(cm < g, cm.astype(np.float64) - np.float64(g), np.inf)
            step_total, pairs, margin = solve(w)
            margin_opt = min(margin_opt, margin)
            needed = max(needed, margin_needed(len(slots), len(listed)))
            total += step_total
            n_pairs += len(pairs)
            assigned = {listed[bi][0]: (slots[si], cm[bi, si]) for bi, si in pairs.items()}
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
                n_new=n_new, n_dropped=n_dropped, state=state, ids=ids_out, next_id=next_id, working=ws, margin_opt=margin_opt,
                margin_gate=margin_gate, margin_needed=needed, total=total, n_pairs=n_pairs)


# ---- cases: all persons of a scene share one joint cloud, so a cost is the distance between centres ---------------------------

def _xyz(v):
    return np.asarray(v, np.float64) if np.ndim(v) else np.array([float(v), 0.0, 3000.0])


def designed(paths, nj=17, capacity=8, seed=0, **params):
    """paths {person: {frame: x or (x, y, z)}} -> follow_tracks_ref.scene with one shared cloud and no noise, the boxes in
    person-major order in memory (so the persons of the first frame are born in their order)."""
    centres = {p: {f: _xyz(v) for f, v in path.items()} for p, path in paths.items()}
    c = FT.scene(centres, nj=nj, capacity=capacity, seed=seed, noise=0.0, shuffle=False, extra_rows=0, **params)
    cloud = np.random.default_rng(seed + 1000).uniform(-300, 300, (nj, 3))
    for i in np.flatnonzero(c['person'] >= 0):
        c['poses'][i] = (centres[int(c['person'][i])][int(round(c['times'][i] * 32.0))] + cloud).astype(np.float32)
    return c


def table_case(slots_x, steps_x, nj=17, capacity=None, seed=0, tie=False, slot_joints=None, box_joints=None, **params):
    """A table that arrives with live slots at rest at slots_x (seen at t = 0, ids = their slots) and steps of boxes at steps_x
    [step][box] (x or (x, y, z)), step j at t = (j + 1) / 32: the first step's cost matrix is min(|slot - box|, clip).
    slot_joints / box_joints {index: joints} restrict a slot's state / a box's finite joints."""
    rng = np.random.default_rng(seed)
    cloud = rng.uniform(-300, 300, (nj, 3)) if nj > 1 else np.zeros((1, 3))
    cap = len(slots_x) if capacity is None else capacity
    state, ids, next_id = FT.new_table(cap, nj)
    for s, x in enumerate(slots_x):
        joints = np.arange(nj) if not slot_joints or s not in slot_joints else np.asarray(slot_joints[s])
        state[s, joints, :3] = (_xyz(x) + cloud)[joints]
        for j in joints:
            state[s, j, 6 + np.array([0, 6, 11])] = 25.0
            state[s, j, 6 + np.array([15, 18, 20])] = 1e4
        state[s, joints, 27] = 0.0
        ids[s] = s
    next_id[0] = len(slots_x)
    boxes = [(j, x) for j, xs in enumerate(steps_x) for x in xs]
    n = len(boxes)
    poses = np.stack([(_xyz(x) + cloud) for _, x in boxes]).astype(np.float32)
    for b, joints in (box_joints or {}).items():
        gone = np.setdiff1d(np.arange(nj), joints)
        poses[b, gone] = np.nan
    times = np.asarray([(j + 1) / 32.0 for j, _ in boxes])
    step_rows, step_starts = FT.time_steps(times)
    isotropic = params.get('measurement') == 'isotropic'
    c = dict(FT.DEFAULTS, poses=poses, cov=None if isotropic else TS._random_cov(rng, (n, nj), sigma=(1.0, 4.0)), times=times,
             step_rows=step_rows, step_starts=step_starts, state=state, ids=ids, next_id=next_id, min_joints=(nj + 1) // 2,
             person=np.arange(n), tie=tie)
    c.update(params)
    return c


def case_trap():
    """The scene of the header: tracks A at 0 and B at 230 mm, then boxes at -120 (A's) and +100 (B's).  Costs A-(+100) 100,
    A-(-120) 120, B-(+100) 130, B-(-120) 350: greedy takes A-(+100) and strands B; the optimum is 120 + 130."""
    return designed({0: {0: 0.0, 1: 0.0, 2: -120.0}, 1: {0: 230.0, 1: 230.0, 2: 100.0}}, seed=61)


def case_not_cardinality():
    """Costs A-p 10, A-q 299, B-p 299, B-q +inf (slot B has a state on joints 0-8 only, box q is finite on joints 8-16 only:
    one joint in common): the single pair at 10 mm (gain 290) beats the two at 299 mm (gain 1 + 1)."""
    return table_case([0.0, 309.0], [[10.0, -299.0]], capacity=4, seed=62, slot_joints={1: range(9)}, box_joints={1: range(8, 17)})


def case_chain():
    """Slots at 0, 250, 500; boxes in step order at 120 (slots 0 / 1 at 120 / 130), 370 (slots 1 / 2 at 120 / 130) and -170 (slot
    0 only, at 170): the third box finds its slot through a path of length 3 that moves both earlier boxes on."""
    return table_case([0.0, 250.0, 500.0], [[120.0, 370.0, -170.0]], capacity=4, seed=63)


def case_all_inadmissible():
    return table_case([0.0, 1000.0], [[400.0, 1500.0, -450.0]], capacity=8, seed=64)


def case_empty_table():
    return designed({0: {0: 0.0, 1: 30.0}, 1: {0: 200.0, 1: 180.0}, 2: {1: 2000.0}}, seed=65)


def case_full_table():
    """Three slots, all live, five boxes: two continue nothing, find no free slot and are counted in n_dropped."""
    return table_case([0.0, 1000.0, 2000.0], [[40.0, 960.0, 2050.0, 3000.0, 4000.0]], seed=66)


def case_tie():
    """J = 1, isotropic, exact in fp32: two slots at x = 0, boxes at +64 and -64: four equal costs of 64."""
    return table_case([0.0, 0.0], [[64.0, -64.0]], nj=1, capacity=4, tie=True, measurement='isotropic', r_floor=2.0, min_joints=1)


def case_tie_chain():
    """J = 1: slots at 0 and 128, boxes at 64 (64 from both) and 192 (64 from slot 1 only): equal path lengths in the search."""
    return table_case([0.0, 128.0], [[64.0, 192.0]], nj=1, capacity=4, tie=True, measurement='isotropic', r_floor=2.0, min_joints=1)


def line_case(n_slots, n_boxes, nj, seed, n_steps=1, capacity=None):
    """Persons on a line 150 mm apart, each stepping 80 to 140 mm along it per step, to either side: box i lies 80-140 mm from
    slot i, 10-70 mm from the neighbour it stepped towards, 160-220 mm from the one after that and 230-290 mm from the
    neighbour behind, so every row of the matrix has up to four admissible columns, its smallest cost is in the wrong one, and
    two persons stepping towards each other or one behind the other compete for the same slots.  Every box also lies up to
    60 mm off the line: costs that were differences of coordinates along one line would tie (|a - x| + |b - y| equals
    |a - y| + |b - x| whenever both boxes lie on one side of both slots)."""
    rng = np.random.default_rng(seed)
    at = 150.0 * np.arange(n_boxes)
    steps = []
    for _ in range(n_steps):
        side = rng.choice([-1.0, 1.0], n_boxes)
        side[0], side[-1] = (1.0, -1.0) if n_boxes > 1 else (side[0], side[0])    # the ends step inwards: three slots in reach
        at = at + side * rng.uniform(80.0, 140.0, n_boxes)
        steps.append([(x, y, 3000.0) for x, y in zip(at, rng.uniform(-60.0, 60.0, n_boxes))])
    kw = dict(measurement='isotropic', r_floor=3.0) if nj == 1 else {}
    return table_case((150.0 * np.arange(n_slots)).tolist(), steps, nj=nj, capacity=capacity, seed=seed, **kw)


def case_stream():
    """Three persons 200 mm apart walking along their line at different speeds for 9 frames, a fourth far away from frame 4."""
    return designed({0: {f: 0.0 + 35.0 * f for f in range(9)}, 1: {f: 200.0 + 12.0 * f for f in range(9)},
                     2: {f: 400.0 - 20.0 * f for f in range(9)}, 3: {f: 3000.0 + 5.0 * f for f in range(4, 9)}}, seed=67)


KNOWN = {
    'trap': case_trap, 'not-cardinality': case_not_cardinality, 'chain': case_chain, 'all-inadmissible': case_all_inadmissible,
    'empty-table': case_empty_table, 'full-table': case_full_table, 'tie': case_tie, 'tie-chain': case_tie_chain, 'stream': case_stream,
}
# live slots T in {1, 2, 64, 65, 128} against boxes m in {1, 2, 63, 64, 65, 128}: m < T, m = T, m > T; J in {1, 17, 64}
LINES = {
    'T1-m1': lambda: line_case(1, 1, 17, 71, capacity=2),
    'T1-m2': lambda: line_case(1, 2, 17, 72, capacity=2),
    'T1-m128-j1': lambda: line_case(1, 128, 1, 73, capacity=128),
    'T2-m1': lambda: line_case(2, 1, 17, 74),
    'T2-m2-j64-steps2': lambda: line_case(2, 2, 64, 75, n_steps=2, capacity=3),
    'T2-m128-j1': lambda: line_case(2, 128, 1, 76, capacity=64),
    'T64-m63': lambda: line_case(64, 63, 17, 77),
    'T64-m64-j1': lambda: line_case(64, 64, 1, 178, capacity=65),
    'T64-m65-j1': lambda: line_case(64, 65, 1, 79),
    'T65-m64-j1': lambda: line_case(65, 64, 1, 80),
    'T65-m128-j1': lambda: line_case(65, 128, 1, 81, capacity=128),
    'T128-m1-j1': lambda: line_case(128, 1, 1, 82),
    'T128-m2-j1': lambda: line_case(128, 2, 1, 83),
    'T128-m63-j1': lambda: line_case(128, 63, 1, 284),
    'T128-m128-j1-steps2': lambda: line_case(128, 128, 1, 85, n_steps=2),
    'T128-m128-j17': lambda: line_case(128, 128, 17, 86),
}
# follow_tracks_ref's scenes under the optimal rule: crossing persons, a slot older than max_age_s among live ones, a box with
# no finite joint, more persons than slots, a retired slot, skipped row indices, and its loop boundaries (65 steps among them)
FOLLOWED = {name: fn for name, fn in FT.CASES.items() if name != 'ties'}
CASES = dict(KNOWN, **LINES, **{'followed-' + name: fn for name, fn in FOLLOWED.items()})


@functools.lru_cache(maxsize=None)
def case_and_expected(name):
    """(case, expected) computed once and shared by the tests of a session: treat both as read-only."""
    c = CASES[name]()
    return c, associate(c)


def compare(got, want, c):
    """follow_tracks_ref.compare; for a case of exact ties only the properties every optimum shares: one slot per box and one
    box per slot, every accepted cost below max_cost, the total within pairs * 1e-3 mm of the optimum's, and the counts."""
    if not c['tie']:
        return FT.compare(got, want, c)
    index, cost = np.asarray(got['track_index']).reshape(-1), np.asarray(got['cost'], np.float32).reshape(-1)
    paired = ~np.isnan(cost)
    assert (index[paired] >= 0).all() and (cost[paired] < np.float32(c['max_cost'])).all()
    tracked = index[index >= 0]
    steps = [[row for _, row in listed] for listed in FT._steps(c)]
    for rows in steps:
        slots = index[rows][index[rows] >= 0]
        assert len(set(slots.tolist())) == len(slots), 'one box per slot and step'
    assert len(tracked) == (want['track_index'] >= 0).sum()
    assert int(paired.sum()) == want['n_pairs']
    total = float((cost[paired].astype(np.float64) - np.float64(np.float32(c['max_cost']))).sum())
    assert abs(total - want['total']) <= max(want['n_pairs'], 1) * COST_MM, (total, want['total'])
    for k in ('n_new', 'n_dropped', 'next_id'):
        assert int(np.asarray(got[k]).reshape(-1)[0]) == want[k], (k, got[k], want[k])
    return abs(total - want['total']), 0.0
