"""fp64 NumPy restatement of metro_triangulate_joints (include/metro_hip.h, metro_pose3d_amd/csrc/triangulate.hip), reading
the same fp32 inputs.  TEST INFRASTRUCTURE: the product never imports it.  It solves every 3x3 system with np.linalg.solve and
tests determinacy with np.linalg.det, where the kernel uses cofactors, and it is vectorised over the rays of a joint where the
kernel adds them one by one: an independent route to the same numbers.

Everything is in the kernel's terms: `perm` maps output joints to head joints, `mirror` is the output-order mirror table
(Skeleton.out_mirror), person p owns the crop rows rows[starts[p]:starts[p+1]]."""
from __future__ import annotations

import numpy as np

UNIFORM, COVARIANCE = 'uniform', 'covariance'
# The rays of a synthetic rig (ring_scene) meet at the truth up to the fp32 rounding of the records and of coords01: cam_loc has
# an ulp of 4.8e-4 mm at 4.5 m, the fp32 rotations give 6e-8 x 5000 mm = 3e-4 mm, coords01 rounds by 1.5e-5 px (6e-5 mm at
# 4.5 m); at a conditioning <= 3 these sum to a few 1e-3 mm.
KNOWN_ANSWER_MM = 1e-2
PARITY_MM = 1e-3                  # two fp64 evaluations of the same fp32 inputs: the project's parity bar for fp64 paths


def pixel_scale(spec):
    """(lrc, half_off) of heatmap_to_image (volumetric.py:288-295): crop pixel = coords01 * lrc + half_off."""
    last = spec.proc_side - 1
    return float(last - last % spec.stride - 1), float(spec.stride // 2 if spec.centered_stride else 0)


def min_det(min_angle_deg):
    return np.sin(np.radians(min_angle_deg)) ** 2 / 4.0


def project(points_world, inv_intrinsics, rot_to_world, cam_loc, spec):
    """World points [..., 3] through ONE crop's virtual camera (the fp32 record fields, taken to fp64) -> coords01 xy [..., 2]
    in fp64: X_virt = rot_to_world^T (X - cam_loc), pixel = K X_virt / z with K = inv(inv_intrinsics)."""
    lrc, half = pixel_scale(spec)
    k = np.linalg.inv(np.asarray(inv_intrinsics, np.float64))
    xv = (np.asarray(points_world, np.float64) - np.asarray(cam_loc, np.float64)) @ np.asarray(rot_to_world, np.float64)
    px = xv @ k.T
    return (px[..., :2] / px[..., 2:] - half) / lrc


def rays(coords01, inv_intrinsics, rot_to_world, cam_loc, perm, mirror, spec):
    """The rays of every (crop row, output joint): (d [m, Jout, 3] unit, o [m, 3], head joint [m, Jout], usable [m, Jout])."""
    lrc, half = pixel_scale(spec)
    c = np.asarray(coords01, np.float32).astype(np.float64)
    k = np.asarray(inv_intrinsics, np.float32).astype(np.float64).reshape(-1, 3, 3)
    r = np.asarray(rot_to_world, np.float32).astype(np.float64).reshape(-1, 3, 3)
    o = np.asarray(cam_loc, np.float32).astype(np.float64).reshape(-1, 3)
    perm, mirror = np.asarray(perm), np.asarray(mirror)
    mirrored = ~(np.linalg.det(r) > 0)
    out = np.arange(len(perm))
    head = np.where(mirrored[:, None], perm[mirror][None, :], perm[out][None, :])              # [m, Jout]
    uv = np.take_along_axis(c[..., :2], head[..., None], axis=1) * lrc + half
    h = np.concatenate([uv, np.ones_like(uv[..., :1])], axis=-1)
    with np.errstate(invalid='ignore', divide='ignore'):
        d = np.einsum('mab,mbc,mjc->mja', r, k, h)
        d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    ok = np.isfinite(d).all(axis=-1) & np.isfinite(o).all(axis=-1)[:, None]
    return d, o, head, ok


def _solve(d, o, w, threshold):
    """Rays d [k, 3], o [k, 3], weights w [k] -> the nearest point, or None when undetermined."""
    if len(d) < 2:
        return None
    proj = np.eye(3)[None] - d[:, :, None] * d[:, None, :]
    a = (w[:, None, None] * proj).sum(axis=0) / w.sum()
    b = (w[:, None] * np.einsum('kab,kb->ka', proj, o)).sum(axis=0) / w.sum()
    if not np.linalg.det(a) >= threshold:
        return None
    return np.linalg.solve(a, b)


def triangulate(coords01, cov01, inv_intrinsics, rot_to_world, cam_loc, rows, starts, perm, mirror, spec, weights=COVARIANCE,
                min_angle_deg=2.0):
    """-> (points float32 [P, Jout, 3], n_rays int32 [P, Jout], residual float32 [P, Jout]) as the kernel defines them."""
    lrc, _ = pixel_scale(spec)
    d, o, head, ok = rays(coords01, inv_intrinsics, rot_to_world, cam_loc, perm, mirror, spec)
    m, n_out = ok.shape
    rows, starts = np.asarray(rows, np.int64), np.asarray(starts, np.int64)
    n_persons = len(starts) - 1
    threshold = min_det(min_angle_deg)
    points = np.full((n_persons, n_out, 3), np.nan, np.float32)
    residual = np.full((n_persons, n_out), np.nan, np.float32)
    n_rays = np.zeros((n_persons, n_out), np.int32)
    if weights == COVARIANCE:
        k0 = np.asarray(inv_intrinsics, np.float32).astype(np.float64).reshape(-1, 3, 3)[:, 0, 0]
        scale = lrc ** 2 * k0 ** 2                                                         # [m]
        cov = np.asarray(cov01, np.float32).astype(np.float64)
    for p in range(n_persons):
        group = rows[max(starts[p], 0):min(starts[p + 1], len(rows))]
        group = group[(group >= 0) & (group < m)]
        for r in range(n_out):
            use = group[ok[group, r]]
            dd, oo = d[use, r], o[use]
            w = np.ones(len(use))
            n_rays[p, r] = len(use)
            x = _solve(dd, oo, w, threshold)
            if x is not None and weights == COVARIANCE:
                j = head[use, r]
                z = np.einsum('ka,ka->k', dd, x[None] - oo)
                s2 = 0.5 * (cov[use, j, 0] + cov[use, j, 1]) * scale[use]
                s2 = np.where(s2 < 1e-12 * scale[use], 1e-12 * scale[use], s2)
                with np.errstate(invalid='ignore', divide='ignore'):
                    w = 1.0 / (s2 * z * z)
                keep = (z > 0) & np.isfinite(w)
                dd, oo, w = dd[keep], oo[keep], w[keep]
                n_rays[p, r] = len(w)
                x = _solve(dd, oo, w, threshold)
            if x is None:
                continue
            v = x[None] - oo
            perp = v - dd * np.einsum('ka,ka->k', dd, v)[:, None]
            points[p, r] = x
            residual[p, r] = np.sqrt((w * (perp ** 2).sum(axis=-1)).sum() / w.sum())
    return points, n_rays, residual


# ---- synthetic rigs: cameras on a ring looking at a cloud of joints ------------------------------------------------------

def ring_cameras(angles_deg, radius=4500.0, height=1200.0, centre=(200.0, -300.0, 1000.0), focal=1150.0, principal=(960.0, 540.0)):
    """One frames.Camera per angle on a ring about `centre`, looking at it (world z is up); the default intrinsics are those of
    1920 x 1080 frames.  Odd cameras carry lens distortion coefficients, even ones none."""
    from metro_pose3d_amd.frames import Camera
    centre = np.asarray(centre, np.float64)
    cams = []
    for k, ang in enumerate(np.radians(angles_deg)):
        t = centre + np.array([radius * np.cos(ang), radius * np.sin(ang), height - centre[2]])
        z = (centre - t) / np.linalg.norm(centre - t)
        x = np.cross(z, [0.0, 0.0, 1.0])
        x /= np.linalg.norm(x)
        rot = np.stack([x, np.cross(z, x), z])
        dist = np.array([-0.12, 0.04, 0.001, -0.0015, 0.005], np.float32) if k % 2 else None
        cams.append(Camera(np.array([[focal, 0, principal[0]], [0, focal * 0.996, principal[1]], [0, 0, 1]]), dist, R=rot, t=t))
    return cams


def ring_scene(angles_deg, n_persons, spec, seed=0, sigma=300.0, radius=4500.0):
    """n_persons clouds of Jout joints (sigma mm about points near the ring's centre) seen by every camera of the ring: one
    box per (person, camera), box-major rows p * n_cams + c.  -> dict(cams, boxes [n, 4], fi [n], pi [n], truth [P, Jout, 3]
    float64, places (frames.PlacementParams of the n crops), coords01 float32 [n, J_head, 3]: every joint projected through
    its crop record's own virtual camera, so the rays meet at the truth up to the fp32 rounding of the records and of
    coords01)."""
    from metro_pose3d_amd import frames as FR
    rng = np.random.default_rng(seed)
    sk = spec.skeleton
    cams = ring_cameras(angles_deg, radius)
    centres = np.array([200.0, -300.0, 1000.0]) + rng.uniform(-400, 400, (n_persons, 3)) * (np.arange(n_persons) > 0)[:, None]
    truth = centres[:, None, :] + rng.normal(0.0, sigma, (n_persons, sk.n_out, 3))
    boxes, fi, pi = [], [], []
    for p in range(n_persons):
        for c, cam in enumerate(cams):
            xc = (truth[p] - cam.t.astype(np.float64)) @ cam.R.astype(np.float64).T
            px = xc[:, :2] / xc[:, 2:] @ cam.intrinsic_matrix[:2, :2].astype(np.float64).T + cam.intrinsic_matrix[:2, 2]
            lo, hi = px.min(axis=0) - 30, px.max(axis=0) + 30
            boxes.append([lo[0], lo[1], hi[0] - lo[0], hi[1] - lo[1]])
            fi.append(c)
            pi.append(p)
    boxes, fi, pi = np.array(boxes), np.array(fi), np.array(pi)
    places = FR.placement_params(cams, boxes, fi, spec.proc_side)
    coords01 = np.zeros((len(boxes), sk.n_head, 3), np.float32)
    perm = np.asarray(sk.permutation)
    for i in range(len(boxes)):
        xy = project(truth[pi[i]], places.inv_intrinsics[i], places.rot_to_world[i], places.cam_loc[i], spec)
        coords01[i, perm, :2] = xy.astype(np.float32)
        coords01[i, perm, 2] = rng.uniform(0, 1, sk.n_out).astype(np.float32)             # depth: not read by the rays
    return dict(cams=cams, boxes=boxes, fi=fi, pi=pi, truth=truth, places=places, coords01=coords01)


def cov01_for(sigma2_px, spec, shape):
    """cov01 [..., 6] whose isotropic pixel variance (cov01_xx + cov01_yy) / 2 . lrc^2 is sigma2_px."""
    lrc, _ = pixel_scale(spec)
    cov = np.zeros(tuple(shape) + (6,), np.float32)
    cov[..., 0] = cov[..., 1] = np.asarray(sigma2_px, np.float64) / lrc ** 2
    cov[..., 2] = 0.01
    return cov


# ---- the cases the kernel is held to, on the host (tests/test_triangulation.py) and on the GPU (test_gpu_triangulation.py) ----

def _take(places, idx):
    return type(places)(*(np.ascontiguousarray(a[idx]) for a in places))


def case(coords01, cov01, places, rows, starts, weights, min_angle_deg=2.0, truth=None, **extra):
    return dict(coords01=np.ascontiguousarray(coords01, np.float32), cov01=np.ascontiguousarray(cov01, np.float32), places=places,
                rows=np.asarray(rows, np.int32), starts=np.asarray(starts, np.int32), weights=weights,
                min_angle_deg=min_angle_deg, truth=truth, **extra)


def expected(c, spec):
    sk, q = spec.skeleton, c['places']
    return triangulate(c['coords01'], c['cov01'], q.inv_intrinsics, q.rot_to_world, q.cam_loc, c['rows'], c['starts'],
                       sk.permutation, sk.out_mirror, spec, c['weights'], c['min_angle_deg'])


def ragged_case(spec, weights, seed=3):
    """4 persons x Jout = 17 joints (68 threads: the launch crosses a 64-thread block) on a 4-camera ring; groups of 2, 3, 4 and
    0 rows; the crop rows stored in a scrambled order and listed in a scrambled order inside each group; noisy coords01
    (2 px) and per-ray variances between 0.5 and 30 px^2, so the two weight modes differ and the residuals are millimetres."""
    rng = np.random.default_rng(seed)
    sk = spec.skeleton
    s = ring_scene([0, 75, 160, 250], 4, spec, seed=seed)
    n, lrc = len(s['boxes']), pixel_scale(spec)[0]
    coords01 = s['coords01'].copy()
    coords01[..., :2] += rng.normal(0, 2.0 / lrc, (n, sk.n_head, 2)).astype(np.float32)
    cov01 = cov01_for(rng.uniform(0.5, 30.0, (n, sk.n_head)), spec, (n, sk.n_head))
    shuffle = rng.permutation(n)                      # stored row k holds box shuffle[k]
    where = np.argsort(shuffle)                       # box i sits in stored row where[i]
    groups = [[0, 1], [4, 5, 6], [8, 9, 10, 11], []]  # box-major: person p, camera c -> box 4 p + c
    rows, starts = [], [0]
    for g in groups:
        rows += list(where[rng.permutation(g)]) if g else []
        starts.append(len(rows))
    return case(coords01[shuffle], cov01[shuffle], _take(s['places'], shuffle), rows, starts, weights)


def flipped_view_case(spec, weights, seed=5):
    """Two persons, three cameras, two views per box: the identity and a horizontal flip (frames.view_params' records; the
    flipped view's rot_to_world has det -1).  A flipped crop shows the person mirrored, so its head joint perm[mirror[r]]
    carries output joint r: its coords01 are built by projecting the MIRROR joints.  A kernel that does not swap left and right
    intersects the rays of different joints and misses the truth by the distance between them (decimetres)."""
    from metro_pose3d_amd import frames as FR
    sk = spec.skeleton
    s = ring_scene([0, 100, 200], 2, spec, seed=seed)
    _, q = FR.view_params(s['cams'], s['boxes'], s['fi'], [(0, 1, False), (0, 1, True)], spec.proc_side)
    n, perm, mirror = len(s['boxes']), np.asarray(sk.permutation), np.asarray(sk.out_mirror)
    coords01 = np.zeros((2 * n, sk.n_head, 3), np.float32)
    for i in range(n):
        for v in range(2):
            row = 2 * i + v
            joints = s['truth'][s['pi'][i]][mirror] if v else s['truth'][s['pi'][i]]
            coords01[row, perm, :2] = project(joints, q.inv_intrinsics[row], q.rot_to_world[row], q.cam_loc[row], spec)
    assert (np.linalg.det(q.rot_to_world[1::2].astype(np.float64)) < 0).all() and (mirror != np.arange(sk.n_out)).any()
    from metro_pose3d_amd.frames import person_groups
    rows, starts = person_groups(s['pi'], s['fi'], 2)
    return case(coords01, cov01_for(1.0, spec, (2 * n, sk.n_head)), q, rows, starts, weights, truth=s['truth'])


def skipped_rays_case(spec, weights, seed=7):
    """One person, four cameras at 0, 90, 180 and 270 degrees, and a fifth row whose camera stands where camera 0 does but looks
    AWAY from the person (camera 0's rotation turned by 180 degrees about its y axis): its rays are finite and enter pass 1,
    but the pass-1 point lies behind it (z <= 0), so pass 2 drops it.  Row 1 holds NaN coords01 for every joint, row 2 for
    joint 3 only; the group also lists the row indices -1 and m, which address no crop.
    -> uniform: n_rays 4 (joint 3: 3), the away-looking ray bends the points; covariance: n_rays 3 (joint 3: 2), the truth."""
    sk = spec.skeleton
    s = ring_scene([0, 90, 180, 270], 1, spec, seed=seed)
    q = _take(s['places'], [0, 1, 2, 3, 0])
    q.rot_to_world[4] = q.rot_to_world[4] @ np.diag([-1.0, 1.0, -1.0]).astype(np.float32)
    coords01 = s['coords01'][[0, 1, 2, 3, 0]].copy()
    coords01[1] = np.nan
    coords01[2, sk.permutation[3]] = np.nan
    return case(coords01, cov01_for(1.0, spec, (5, sk.n_head)), q, [4, -1, 0, 1, 5, 2, 3], [0, 7], weights, truth=s['truth'])


def determinacy_case(spec, weights, min_angle_deg=2.0, seed=9):
    """Person 0: two cameras 1 degree apart (every joint's rays nearly parallel).  Person 1: two cameras 90 degrees apart, but
    joint 5 has NaN coords01 in one of them (one ray left).  Person 2: one row.  Person 3: no rows."""
    sk = spec.skeleton
    a = ring_scene([0, 1], 1, spec, seed=seed)
    b = ring_scene([30, 120], 1, spec, seed=seed + 1)
    coords01 = np.concatenate([a['coords01'], b['coords01']])
    coords01[3, sk.permutation[5]] = np.nan
    places = type(a['places'])(*(np.concatenate([x, y]) for x, y in zip(a['places'], b['places'])))
    return case(coords01, cov01_for(1.0, spec, (4, sk.n_head)), places, [0, 1, 2, 3, 2], [0, 2, 4, 5, 5], weights, min_angle_deg,
                truth=np.concatenate([a['truth'], b['truth']]))


def compare(got, want, bound_mm):
    """(points, n_rays, residual) of the code under test against the restatement's: the same ray counts, the same NaN pattern
    (which also shows every output was written: the callers pre-fill them with a sentinel), points and residuals within
    bound_mm.  -> (worst point deviation, worst residual deviation) in mm."""
    (gp, gn, gr), (wp, wn, wr) = [tuple(np.asarray(a) for a in t) for t in (got, want)]
    assert gp.shape == wp.shape and gn.shape == wn.shape and gr.shape == wr.shape
    assert np.array_equal(gn, wn), (gn, wn)
    assert np.array_equal(np.isnan(gp), np.isnan(wp)) and np.array_equal(np.isnan(gr), np.isnan(wr))
    assert np.array_equal(np.isnan(gp).any(axis=-1), np.isnan(gr))
    worst = [float(np.nanmax(np.abs(g.astype(np.float64) - w), initial=0.0)) for g, w in ((gp, wp), (gr, wr))]
    assert worst[0] <= bound_mm and worst[1] <= bound_mm, worst
    return worst


def check_case(name, c, got, known_answer_mm):
    """What each case is there to show, on the outputs of the code under test."""
    points, n_rays, residual = (np.asarray(a) for a in got)
    weighted = c['weights'] == COVARIANCE
    if name == 'ragged':
        assert (n_rays == np.array([2, 3, 4, 0])[:, None]).all()
        assert np.isfinite(points[:3]).all() and np.isnan(points[3]).all() and np.isnan(residual[3]).all()
        assert residual[:3].min() > 0.01                              # noisy rays do not meet
    elif name == 'flipped-view':
        assert (n_rays == 6).all() and np.abs(points - c['truth']).max() <= known_answer_mm
    elif name == 'skipped-rays':
        usable = np.full(points.shape[1], 3 if weighted else 4)
        usable[3] -= 1
        assert (n_rays[0] == usable).all() and np.isfinite(points).all() and np.isfinite(residual).all()
        if weighted:
            assert np.abs(points - c['truth']).max() <= known_answer_mm
        else:
            assert np.abs(points - c['truth']).max() > 10             # the away-looking ray is in the uniform solve
    elif name.startswith('determinacy'):
        nan = np.isnan(points).all(axis=-1)
        assert nan[0].all() == (c['min_angle_deg'] >= 2.0) and np.isfinite(points[0]).all() == (c['min_angle_deg'] < 1.0)
        assert (n_rays[0] == 2).all()
        assert nan[1].sum() == 1 and nan[1, 5] and n_rays[1, 5] == 1
        assert np.abs(np.delete(points[1] - c['truth'][1], 5, axis=0)).max() <= known_answer_mm
        assert nan[2].all() and (n_rays[2] == 1).all() and nan[3].all() and (n_rays[3] == 0).all()
    else:
        raise KeyError(name)


CASES = {'ragged': ragged_case, 'flipped-view': flipped_view_case, 'skipped-rays': skipped_rays_case,
         'determinacy': determinacy_case,
         'determinacy-half-degree': lambda spec, weights: determinacy_case(spec, weights, min_angle_deg=0.5)}
