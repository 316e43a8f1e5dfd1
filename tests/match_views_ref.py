"""fp64 NumPy restatement of metro_view_affinity and metro_cluster_views (include/metro_hip.h,
metro_pose3d_amd/csrc/match_views.hip), reading the same fp32 inputs.  TEST INFRASTRUCTURE: the product never imports it.
An independent route to the same numbers: the rays are built here from the placement records (not by the triangulation
restatement), the closest approach of two rays is the least-squares solution of the 3x2 system [da, -db] (ta, tb) = ob - oa
(np.linalg.lstsq) where the kernel uses the closed form, and the clustering keeps plain Python sets of boxes and recomputes
every cluster-pair maximum from the ORIGINAL matrix in every round where the kernel updates its working matrix in place.

The rigs and case builders of tests/triangulation_ref.py (ring_cameras, project, cov01_for) are reused."""
from __future__ import annotations

import numpy as np

from tests import triangulation_ref as TR

UNIFORM, COVARIANCE = TR.UNIFORM, TR.COVARIANCE
KNOWN_ANSWER_MM = TR.KNOWN_ANSWER_MM        # the rays of an exact rig pass within the fp32 rounding of the records (see there)
PARITY_MM = TR.PARITY_MM                    # two fp64 evaluations of the same fp32 inputs
MAX_COST_MM, CLIP_MM = 200.0, 500.0         # the defaults of frames.match_poses_in_frames
MAX_BOXES = 128


# ---- metro_view_affinity -------------------------------------------------------------------------------------------------

def _ray(c01, k_inv, rot, loc, head_joint, lrc, half):
    """One ray: (unit direction or None, origin) in fp64 from the fp32 record fields."""
    uv1 = np.array([c01[head_joint, 0] * lrc + half, c01[head_joint, 1] * lrc + half, 1.0])
    with np.errstate(invalid='ignore', divide='ignore'):
        d = rot @ (k_inv @ uv1)
        d = d / np.sqrt(d @ d)
    if not (np.isfinite(d).all() and np.isfinite(loc).all()):
        return None, loc
    return d, loc


def closest_approach(da, oa, db, ob):
    """(ta, tb, dist) of the lines oa + ta da and ob + tb db by least squares: minimise |oa + ta da - ob - tb db|."""
    sol = np.linalg.lstsq(np.stack([da, -db], axis=1), ob - oa, rcond=None)[0]
    gap = (oa + sol[0] * da) - (ob + sol[1] * db)
    return float(sol[0]), float(sol[1]), float(np.sqrt(gap @ gap))


def affinity(coords01, cov01, inv_intrinsics, rot_to_world, cam_loc, frame_index, perm, mirror, spec, n_views=1,
             weights=COVARIANCE, min_angle_deg=2.0, clip_mm=CLIP_MM, min_pairs=None):
    """-> (cost float32 [n, n], n_pairs int32 [n, n]) as the kernel defines them; min_pairs None: ((Jout + 1) // 2) n_views."""
    lrc, half = TR.pixel_scale(spec)
    c = np.asarray(coords01, np.float32).astype(np.float64)
    k = np.asarray(inv_intrinsics, np.float32).astype(np.float64).reshape(-1, 3, 3)
    rot = np.asarray(rot_to_world, np.float32).astype(np.float64).reshape(-1, 3, 3)
    loc = np.asarray(cam_loc, np.float32).astype(np.float64).reshape(-1, 3)
    fi = np.asarray(frame_index).reshape(-1)
    perm, mirror = list(perm), list(mirror)
    n, n_out = len(fi), len(perm)
    assert len(c) == n * n_views
    if min_pairs is None:
        min_pairs = ((n_out + 1) // 2) * n_views
    min_sin2 = np.sin(np.radians(min_angle_deg)) ** 2
    covariance = weights == COVARIANCE
    if covariance:
        cov = np.asarray(cov01, np.float32).astype(np.float64)
    rays = {}
    for row in range(n * n_views):
        flipped = not np.linalg.det(rot[row]) > 0
        for r in range(n_out):
            j = perm[mirror[r]] if flipped else perm[r]
            d, o = _ray(c[row], k[row], rot[row], loc[row], j, lrc, half)
            s2 = 0.0
            if covariance:
                scale = lrc ** 2 * k[row, 0, 0] ** 2
                s2 = 0.5 * (cov[row, j, 0] + cov[row, j, 1]) * scale
                if s2 < 1e-12 * scale:
                    s2 = 1e-12 * scale
            rays[row, r] = (d, o, s2)
    cost = np.full((n, n), np.inf, np.float32)
    n_pairs = np.zeros((n, n), np.int32)
    for a in range(n):
        for b in range(a + 1, n):
            if fi[a] == fi[b]:
                continue
            num = den = 0.0
            cnt = 0
            for v in range(n_views):
                for r in range(n_out):
                    (da, oa, sa), (db, ob, sb) = rays[a * n_views + v, r], rays[b * n_views + v, r]
                    if da is None or db is None or 1.0 - (da @ db) ** 2 < min_sin2:
                        continue
                    ta, tb, dist = closest_approach(da, oa, db, ob)
                    dist = clip_mm if ta <= 0 or tb <= 0 else min(dist, clip_mm)
                    w = 1.0
                    if covariance:
                        with np.errstate(invalid='ignore', divide='ignore'):
                            w = np.float64(1.0) / (sa * ta ** 2 + sb * tb ** 2)
                        if not (np.isfinite(w) and w > 0):
                            continue
                    num += w * dist ** 2
                    den += w
                    cnt += 1
            n_pairs[a, b] = n_pairs[b, a] = cnt
            if cnt >= min_pairs:
                cost[a, b] = cost[b, a] = np.sqrt(num / den)
    return cost, n_pairs


# ---- metro_cluster_views ---------------------------------------------------------------------------------------------------

def cluster(cost, max_cost, n_views=1):
    """-> (person_index int32 [n], n_persons, rows int32 [n n_views], starts int32 [n + 1]) as the kernel defines them."""
    c = np.asarray(cost, np.float32).astype(np.float64)
    n = len(c)
    c = np.where(np.isnan(c), np.inf, c)
    c = np.maximum(c, c.T)
    clusters = [{i} for i in range(n)]
    while True:
        best = None
        for x in sorted(clusters, key=min):
            for y in sorted(clusters, key=min):
                if min(x) < min(y):
                    value = max(c[i, j] for i in x for j in y)            # complete linkage, from the original matrix
                    if best is None or value < best[0]:                   # strict: ties stay with the first (a, b)
                        best = (value, x, y)
        if best is None or not best[0] < max_cost:
            break
        clusters.remove(best[2])
        best[1].update(best[2])
    clusters.sort(key=min)
    person_index = np.zeros(n, np.int32)
    rows, starts = [], [0]
    for p, boxes in enumerate(clusters):
        person_index[sorted(boxes)] = p
        if len(boxes) > 1:
            rows += [i * n_views + v for i in sorted(boxes) for v in range(n_views)]
        starts.append(len(rows))
    starts += [len(rows)] * (n - len(clusters))
    rows += [-1] * (n * n_views - len(rows))
    return person_index, len(clusters), np.asarray(rows, np.int32).reshape(-1), np.asarray(starts, np.int32)


def single_linkage(cost, max_cost):
    """Labels of the connected components of cost < max_cost: what complete linkage must NOT give on the chain case."""
    c = np.asarray(cost, np.float64)
    n = len(c)
    label = list(range(n))
    for _ in range(n):
        for a in range(n):
            for b in range(n):
                if max(c[a, b], c[b, a]) < max_cost:
                    label[a] = label[b] = min(label[a], label[b])
    return label


def _sym(n, entries, fill=np.inf):
    c = np.full((n, n), fill, np.float32)
    for (a, b), v in entries.items():
        c[a, b] = c[b, a] = v
    return c


def _frames_for(cost):
    """Frame indices under which every +inf (or NaN) entry off the diagonal is a same-frame pair where that is possible: boxes
    joined by such an entry share a frame (connected components); the callers' matrices are built so that no finite entry
    joins two boxes of one component."""
    c = np.asarray(cost, np.float64)
    c = np.maximum(np.where(np.isnan(c), np.inf, c), np.where(np.isnan(c.T), np.inf, c.T))
    n = len(c)
    frame = list(range(n))
    for _ in range(n):
        for a in range(n):
            for b in range(n):
                if a != b and np.isinf(c[a, b]):
                    frame[a] = frame[b] = min(frame[a], frame[b])
    return np.asarray(frame, np.int64)


def cluster_cases():
    """Hand-made matrices: name -> (cost, max_cost, n_views, the labels the case is there to show)."""
    cases = {}
    # exact ties (every value a small integer): (0, 1) and (0, 2) tie at 4 -> the lowest b merges, after which 2 is 16 away
    cases['tie-b'] = (_sym(3, {(0, 1): 4.0, (0, 2): 4.0, (1, 2): 16.0}), 8.0, 1, [0, 0, 1])
    # (0, 2) and (1, 2) tie at 4 -> the lowest a merges, after which 1 is 16 away
    cases['tie-a'] = (_sym(3, {(0, 2): 4.0, (1, 2): 4.0, (0, 1): 16.0}), 8.0, 1, [0, 1, 0])
    # two tied pairs that do not touch: both merge, (0, 2) first, and the merged clusters stay apart
    cases['tie-both'] = (_sym(4, {(0, 2): 8.0, (1, 3): 8.0, (0, 1): 64.0, (0, 3): 32.0, (1, 2): 32.0, (2, 3): 64.0}), 48.0, 1,
                         [0, 1, 0, 1])
    # a chain: A-B and B-C close, A-C far: complete linkage joins A-B (the closer pair) and leaves C
    cases['chain'] = (_sym(3, {(0, 1): 10.0, (1, 2): 12.0, (0, 2): 300.0}), 200.0, 1, [0, 0, 1])
    # boxes 0 and 1 share a frame (+inf); 2 is close to both: it joins 0 (the closer), and 1 must stay out through the merge
    cases['inf-propagates'] = (_sym(4, {(0, 2): 5.0, (1, 2): 6.0, (0, 3): 7.0, (1, 3): 150.0, (2, 3): 9.0}), 200.0, 2, [0, 1, 0, 0])
    cases['equal-to-max'] = (_sym(3, {(0, 1): 200.0, (0, 2): 250.0, (1, 2): 199.99998474121094}), 200.0, 1, [0, 1, 1])
    nan = _sym(4, {(0, 1): 3.0, (2, 3): 4.0, (0, 2): 500.0, (1, 3): 500.0, (0, 3): 500.0, (1, 2): 500.0})
    nan[0, 1] = np.nan                                                   # one side NaN: the pair reads +inf
    nan[3, 2] = 4.0
    cases['nan'] = (nan, 200.0, 1, [0, 1, 2, 2])
    asym = _sym(3, {(0, 1): 10.0, (0, 2): 400.0, (1, 2): 20.0})
    asym[1, 0] = 250.0                                                   # max(10, 250) = 250: not merged
    cases['asymmetric'] = (asym, 200.0, 3, [0, 1, 1])
    cases['all-inf'] = (np.full((5, 5), np.inf, np.float32), 200.0, 2, [0, 1, 2, 3, 4])
    cases['n1'] = (np.full((1, 1), np.inf, np.float32), 200.0, 2, [0])
    # 128 boxes: 32 persons x 4 cameras in scrambled order; same person 1 + (p mod 7), others 300 + ..., same camera +inf
    rng = np.random.default_rng(11)
    order = rng.permutation(128)
    person, camera = order // 4, order % 4
    big = np.where(person[:, None] == person[None, :], 1.0 + (person[:, None] % 7), 300.0 + np.abs(person[:, None] - person[None, :]))
    big = np.where(camera[:, None] == camera[None, :], np.inf, big).astype(np.float32)
    first = {}
    cases['n128'] = (big, 200.0, 1, [first.setdefault(p, len(first)) for p in person])
    return cases


def random_cost(n, seed, inf_fraction=0.15, scale=400.0):
    """A symmetric matrix of DISTINCT finite fp32 values with a sprinkling of +inf pairs (and an +inf diagonal)."""
    rng = np.random.default_rng(seed)
    values = (rng.permutation(n * n).astype(np.float64) + 1.0) * (scale / (n * n))         # distinct, exactly spaced
    c = np.triu(values.reshape(n, n), 1)
    c = np.where(np.triu(rng.uniform(size=(n, n)) < inf_fraction, 1), np.inf, c)
    c = c + c.T
    np.fill_diagonal(c, np.inf)
    c = c.astype(np.float32)
    finite = c[np.triu_indices(n, 1)]
    finite = finite[np.isfinite(finite)]
    assert len(np.unique(finite)) == len(finite)
    return c


def compare_clusters(got, want):
    """All four outputs of the code under test equal the restatement's."""
    for g, w, name in zip(got, want, ('person_index', 'n_persons', 'rows', 'starts')):
        g, w = np.asarray(g).reshape(-1), np.asarray(w).reshape(-1)
        assert g.shape == w.shape and np.array_equal(g, w), (name, g, w)


# ---- rigs: persons on a grid seen by a ring of cameras ---------------------------------------------------------------------

def rig_scene(angles_deg, n_persons, spec, seed=0, spacing=700.0, sigma=300.0, order=None, drop=(), views=1):
    """n_persons clouds of Jout joints (sigma mm) about centres `spacing` mm apart on a grid near the ring's centre, seen by
    every camera of TR.ring_cameras(angles_deg): one box per (camera, person), CAMERA-major as a detector run per camera gives
    them, then reordered by `order` (a permutation) and with the boxes listed in `drop` (indices after the reordering) left
    out.  views=2: an identity and a flipped view per box (frames.view_params), the flipped one built from the mirror joints.
    -> dict(cams, boxes, fi, pi, truth [P, Jout, 3], centres [P, 3], places (n * views records), coords01 float32
    [n * views, J_head, 3] exact projections, n_views)."""
    from metro_pose3d_amd import frames as FR
    rng = np.random.default_rng(seed)
    sk = spec.skeleton
    cams = TR.ring_cameras(angles_deg)
    side = int(np.ceil(np.sqrt(n_persons)))
    grid = np.array([[(p % side) - (side - 1) / 2, (p // side) - (side - 1) / 2, 0.0] for p in range(n_persons)]) * spacing
    centres = np.array([200.0, -300.0, 1000.0]) + grid
    truth = centres[:, None, :] + rng.normal(0.0, sigma, (n_persons, sk.n_out, 3))
    boxes, fi, pi = [], [], []
    for c, cam in enumerate(cams):
        for p in range(n_persons):
            xc = (truth[p] - cam.t.astype(np.float64)) @ cam.R.astype(np.float64).T
            px = xc[:, :2] / xc[:, 2:] @ cam.intrinsic_matrix[:2, :2].astype(np.float64).T + cam.intrinsic_matrix[:2, 2]
            lo, hi = px.min(axis=0) - 30, px.max(axis=0) + 30
            boxes.append([lo[0], lo[1], hi[0] - lo[0], hi[1] - lo[1]])
            fi.append(c)
            pi.append(p)
    keep = np.arange(len(boxes)) if order is None else np.asarray(order)
    keep = np.delete(keep, list(drop))
    boxes, fi, pi = np.array(boxes)[keep], np.array(fi)[keep], np.array(pi)[keep]
    n, perm, mirror = len(boxes), np.asarray(sk.permutation), np.asarray(sk.out_mirror)
    if views == 1:
        places = FR.placement_params(cams, boxes, fi, spec.proc_side)
    else:
        assert views == 2
        places = FR.view_params(cams, boxes, fi, [(0, 1, False), (0, 1, True)], spec.proc_side)[1]
    coords01 = np.zeros((n * views, sk.n_head, 3), np.float32)
    for i in range(n):
        for v in range(views):
            row = i * views + v
            joints = truth[pi[i]][mirror] if v else truth[pi[i]]
            coords01[row, perm, :2] = TR.project(joints, places.inv_intrinsics[row], places.rot_to_world[row], places.cam_loc[row],
                                                 spec).astype(np.float32)
            coords01[row, perm, 2] = rng.uniform(0, 1, sk.n_out).astype(np.float32)        # depth: not read by the rays
    return dict(cams=cams, boxes=boxes, fi=fi, pi=pi, truth=truth, centres=centres, places=places, coords01=coords01, n_views=views)


def case(s, spec, weights, noise_px=0.0, seed=0, **extra):
    """A kernel case from a rig scene: coords01 (plus noise_px of noise), per-ray variances between 0.5 and 30 px^2 so that the
    two weight modes differ, and the launch's parameters (defaults: the product's)."""
    rng = np.random.default_rng(1000 + seed)
    sk = spec.skeleton
    m, lrc = len(s['coords01']), TR.pixel_scale(spec)[0]
    coords01 = s['coords01'].copy()
    if noise_px:
        coords01[..., :2] += rng.normal(0, noise_px / lrc, (m, sk.n_head, 2)).astype(np.float32)
    cov01 = TR.cov01_for(rng.uniform(0.5, 30.0, (m, sk.n_head)), spec, (m, sk.n_head))
    c = dict(coords01=np.ascontiguousarray(coords01), cov01=np.ascontiguousarray(cov01), places=s['places'],
             fi=np.asarray(s['fi'], np.int32), pi=np.asarray(s['pi']), n_views=s['n_views'], weights=weights, min_angle_deg=2.0,
             clip_mm=CLIP_MM, min_joints=None)
    c.update(extra)
    return c


def min_pairs_of(c, spec):
    mj = (spec.skeleton.n_out + 1) // 2 if c['min_joints'] is None else c['min_joints']
    return mj * c['n_views']


def expected(c, spec):
    sk, q = spec.skeleton, c['places']
    return affinity(c['coords01'], c['cov01'], q.inv_intrinsics, q.rot_to_world, q.cam_loc, c['fi'], sk.permutation, sk.out_mirror,
                    spec, c['n_views'], c['weights'], c['min_angle_deg'], c['clip_mm'], min_pairs_of(c, spec))


def _rig_case(angles, persons, seed, **kw):
    return lambda spec, weights: case(rig_scene(angles, persons, spec, seed=seed, **kw), spec, weights, noise_px=2.0, seed=seed)


def _scrambled(spec, weights):
    order = np.random.default_rng(4).permutation(12)
    return case(rig_scene([0, 70, 140, 230], 3, spec, seed=4, order=order), spec, weights, noise_px=2.0, seed=4)


def _flipped(spec, weights):
    return case(rig_scene([0, 100, 200], 2, spec, seed=5, views=2), spec, weights, noise_px=1.0, seed=5)


def _nan_joint(spec, weights):
    c = case(rig_scene([0, 120, 240], 2, spec, seed=6), spec, weights, noise_px=2.0, seed=6)
    c['coords01'][1, spec.skeleton.permutation[3]] = np.nan            # box 1: output joint 3 has no ray
    if weights == COVARIANCE:
        c['cov01'][2, spec.skeleton.permutation[5], :2] = np.nan        # box 2: joint 5 has no weight
    return c


def _near_parallel(spec, weights):
    """Cameras 0 and 1 stand 1 degree apart: every ray pair between their boxes is within 2 degrees of parallel."""
    return case(rig_scene([0, 1, 90], 1, spec, seed=7), spec, weights, noise_px=1.0, seed=7)


def _behind_camera(spec, weights):
    """Box 1's camera is turned away from the person (180 degrees about its y axis): its rays meet every other ray behind it."""
    s = rig_scene([0, 90, 200], 1, spec, seed=8)
    s['places'].rot_to_world[1] = s['places'].rot_to_world[1] @ np.diag([-1.0, 1.0, -1.0]).astype(np.float32)
    return case(s, spec, weights, seed=8)


def _too_few(spec, weights):
    """Box 0 keeps 8 of its 17 joints (fewer than the default 9); with min_joints = 8 the same pairs would count."""
    c = case(rig_scene([0, 90, 200], 2, spec, seed=9), spec, weights, noise_px=2.0, seed=9)
    perm = np.asarray(spec.skeleton.permutation)
    c['coords01'][0, perm[8:]] = np.nan
    return c


def _one_frame(spec, weights):
    c = case(rig_scene([0, 90], 1, spec, seed=10), spec, weights, seed=10)
    c['fi'][:] = 1                                                       # both boxes declared on one frame
    return c


def _single(spec, weights):
    return case(rig_scene([0], 1, spec, seed=11), spec, weights, seed=11)


CASES = {
    'rig-2x1': _rig_case([0, 90], 1, 21), 'rig-2x3': _rig_case([0, 90], 3, 22), 'rig-3x5': _rig_case([0, 120, 240], 5, 23),
    'rig-4x2': _rig_case([0, 70, 140, 230], 2, 24), 'rig-4x4': _rig_case([0, 70, 140, 230], 4, 25),
    'scrambled': _scrambled, 'missing': _rig_case([0, 120, 240], 3, 26, drop=(4,)), 'one-frame': _one_frame, 'flipped-views': _flipped,
    'nan-joint': _nan_joint, 'near-parallel': _near_parallel, 'behind-camera': _behind_camera, 'too-few': _too_few, 'n1': _single,
}


def compare(got, want, bound_mm):
    """(cost, n_pairs) of the code under test against the restatement's: equal pair counts, +inf at the same entries (which
    also shows that every entry was written: the callers pre-fill the outputs with a sentinel), finite costs within bound_mm.
    -> the worst deviation in mm."""
    (gc, gn), (wc, wn) = [tuple(np.asarray(a) for a in t) for t in (got, want)]
    assert gc.shape == wc.shape and gn.shape == wn.shape and gc.dtype == np.float32 and gn.dtype == np.int32
    assert np.array_equal(gn, wn), (gn, wn)
    assert not np.isnan(gc).any() and np.array_equal(np.isposinf(gc), np.isposinf(wc)), (gc, wc)
    assert np.array_equal(gc, gc.T) and np.array_equal(gn, gn.T)
    finite = np.isfinite(wc)
    worst = float(np.abs(gc[finite].astype(np.float64) - wc[finite]).max(initial=0.0))
    assert worst <= bound_mm, worst
    return worst


def check_case(name, c, got, spec):
    """What each case is there to show, on the outputs of the code under test."""
    cost, n_pairs = (np.asarray(a) for a in got)
    n, full = len(c['fi']), spec.skeleton.n_out * c['n_views']
    same_frame = c['fi'][:, None] == c['fi'][None, :]
    assert np.isposinf(cost[same_frame]).all() and (n_pairs[same_frame] == 0).all()
    if name.startswith('rig') or name in ('scrambled', 'missing', 'flipped-views'):
        assert (n_pairs[~same_frame] == full).all() and np.isfinite(cost[~same_frame]).all()
        same_person = (c['pi'][:, None] == c['pi'][None, :]) & ~same_frame
        assert cost[same_person].max() < 50.0                          # 2 px (1 px) of noise at 4.5 m: centimetres
        if name == 'missing':
            assert n == 8 and np.bincount(c['pi']).tolist() == [3, 2, 3]
    elif name == 'one-frame':
        assert np.isposinf(cost).all() and (n_pairs == 0).all()
    elif name == 'nan-joint':
        weighted = c['weights'] == COVARIANCE
        for a in range(n):
            for b in range(n):
                if not same_frame[a, b]:
                    assert n_pairs[a, b] == full - (1 in (a, b)) - (weighted and 2 in (a, b)), (a, b)
    elif name == 'near-parallel':
        assert n_pairs[0, 1] == 0 and np.isposinf(cost[0, 1]) and n_pairs[0, 2] == full and n_pairs[1, 2] == full
        assert np.isfinite(cost[0, 2]) and np.isfinite(cost[1, 2])
    elif name == 'behind-camera':
        assert n_pairs[0, 1] == full and n_pairs[1, 2] == full and cost[0, 1] == c['clip_mm'] and cost[1, 2] == c['clip_mm']
        assert cost[0, 2] <= KNOWN_ANSWER_MM
    elif name == 'too-few':
        others = np.flatnonzero(c['fi'] != c['fi'][0])
        assert (n_pairs[0, others] == 8).all() and np.isposinf(cost[0, others]).all()
        rest = ~same_frame
        rest[0, :] = rest[:, 0] = False
        assert (n_pairs[rest] == full).all() and np.isfinite(cost[rest]).all()
    elif name == 'n1':
        assert cost.shape == (1, 1) and np.isposinf(cost[0, 0]) and n_pairs[0, 0] == 0
    else:
        raise KeyError(name)
