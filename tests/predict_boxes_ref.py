"""fp64 NumPy restatement of metro_predict_boxes, written from the header comment of include/metro_hip.h: the yardstick of
tests/test_predict_boxes.py (the kernel's code compiled for the host) and tests/test_gpu_predict_boxes.py (the launch).  Nothing
in the reference to compare with: one example is one image and its box is given.  Deliberately unlike the kernel: the
prediction is a dense 6x6 F P F^T + Q (tests/track_smoothing_ref.py's matrices), the cameras are frames.Camera objects and not
the packed table, the projection runs on np.float32 arrays of all joints of a slot at once in project_points' statement order,
the compaction appends to Python lists, and the overlap is taken on corner intervals (x0, y0, x1, y1).

Besides the outputs, `predict` reports how far every decision of a case is from flipping (`margins`), so that the tests can show
that the tolerance of the comparison cannot change one.  Also the cases both test files run."""
import functools

import numpy as np

from metro_pose3d_amd.camera import Camera
from tests import track_smoothing_ref as TS

SENTINEL = -7
BOX_PX = 1e-2              # bound of the comparison, pixels, on frames up to LIMIT_PX
LIMIT_PX = 4096
# every decision of a compared case is at least this far from flipping
MARGIN_PX, MARGIN_MM, MARGIN_SLOPE, MARGIN_IOU, MARGIN_AGE_S = 1e-1, 1e-1, 1e-3, 1e-2, 1e-3
DEFAULTS = dict(q=4e6, max_age=1.0, expand=1.25, n_sigma=2.0, max_sigma=300.0, near=100.0, min_side=8.0, min_joints=None,
                clip=True, iou_max=0.3)


def params_of(c):
    p = {**DEFAULTS, **c.get('params', {})}
    if p['min_joints'] is None:
        p['min_joints'] = (c['state'].shape[1] + 1) // 2
    return p


def advance(s28, t, q):
    """One joint's state at time t: (position [3], its covariance [3, 3]) of x- = F x, P- = F P F^T + Q."""
    x, p, t_last = TS.unpack_state(s28)
    f, qm = TS._transition(TS._step_dt(t, t_last), q)
    return (f @ x)[:3], (f @ p @ f.T + qm)[:3, :3]


def pixels(cam, pc):
    """fp64 camera points [k, 3] -> float32 pixels [k, 2]: the points rounded to float32, then project_points' statements on
    float32 arrays (with coefficients), or K (x/z, y/z, 1) in float32."""
    p = pc.astype(np.float32)
    xy = p[:, :2] / p[:, 2:]
    k = cam.intrinsic_matrix.astype(np.float32)
    if cam.distortion_coeffs is not None:
        d = cam.distortion_coeffs.astype(np.float32)
        two = np.float32(2)
        r2 = xy[:, 0] * xy[:, 0] + xy[:, 1] * xy[:, 1]
        r4 = r2 * r2
        dist = d[0] * r2
        dist = dist + d[1] * r4
        r6 = r4 * r2
        dist = dist + d[4] * r6
        dist = dist + np.float32(1)
        dist = dist + xy[:, 0] * (two * d[3])
        dist = dist + xy[:, 1] * (two * d[2])
        xy = np.stack([xy[:, 0] * dist + r2 * d[3], xy[:, 1] * dist + r2 * d[2]], axis=1)
    u = (k[0, 0] * xy[:, 0] + k[0, 1] * xy[:, 1]) + k[0, 2]
    v = (k[1, 0] * xy[:, 0] + k[1, 1] * xy[:, 1]) + k[1, 2]
    assert u.dtype == np.float32 and v.dtype == np.float32
    return np.stack([u, v], axis=1)


def overlap(a, b):
    """Intersection over union of two corner boxes (x0, y0, x1, y1)."""
    ix = max(0.0, min(a[2], b[2]) - max(a[0], b[0]))
    iy = max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
    inter = ix * iy
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def _corners(b):
    return (b[0], b[1], b[0] + b[2], b[1] + b[3])


def predict(c):
    """The case -> dict(boxes [n, 4], frame, slot, id, detection, n_joints int [n], counts [5], dense_boxes [F, T, 4],
    dense_joints [F, T], margins).  margins: the smallest distance of any decision of the case from flipping -- 'near_mm' (z
    against near_mm), 'slope' (the monotonic-range polynomial against 0), 'side_px' (a side against min_side_px, for every slot
    with enough joints), 'iou' (against iou_max, every valid detection against every predicted box of its frame), 'age_s'
    (against max_age_s, every live slot); inf where the case takes no such decision."""
    p = params_of(c)
    state, ids = np.asarray(c['state'], np.float64), np.asarray(c['ids'])
    n_tracks, nj = state.shape[:2]
    cams, sizes, times = c['cameras'], np.asarray(c['sizes']), np.asarray(c['times'], np.float64)
    n_frames = len(times)
    dense = np.full((n_frames, n_tracks, 4), np.nan)
    dense_joints = np.full((n_frames, n_tracks), -1, np.int32)
    margins = dict(near_mm=np.inf, slope=np.inf, side_px=np.inf, iou=np.inf, age_s=np.inf)

    def closer(key, distance):
        margins[key] = min(margins[key], abs(float(distance)))

    for f in range(n_frames):
        cam = cams[0] if len(cams) == 1 else cams[f]
        focal = np.sqrt(abs(float(cam.intrinsic_matrix[0, 0]) * float(cam.intrinsic_matrix[1, 1])))
        for s in range(n_tracks):
            have = [j for j in range(nj) if not np.isnan(state[s, j, 27])]
            if ids[s] < 0 or not have:
                continue
            age = times[f] - max(state[s, j, 27] for j in have)
            closer('age_s', age - p['max_age'])
            if age > p['max_age']:
                continue
            moved = [advance(state[s, j], times[f], p['q']) for j in have]
            pos = np.stack([m[0] for m in moved])
            var = np.array([max(np.diag(m[1]).max(), 0.0) for m in moved])
            if c['coords'] == 'world':
                pos = (pos - cam.t.astype(np.float64)) @ cam.R.astype(np.float64).T
            ok = np.isfinite(pos).all(axis=1)
            with np.errstate(all='ignore'):
                for z in pos[ok, 2]:
                    closer('near_mm', z - p['near'])
                ok &= pos[:, 2] >= p['near']
                if cam.distortion_coeffs is not None:
                    k1, k2, _, _, k3 = (float(v) for v in cam.distortion_coeffs)
                    r2 = (pos[:, 0] / pos[:, 2]) ** 2 + (pos[:, 1] / pos[:, 2]) ** 2
                    slope = 1 + 3 * k1 * r2 + 5 * k2 * r2 ** 2 + 7 * k3 * r2 ** 3
                    for v in slope[ok]:
                        closer('slope', v)
                    ok &= slope > 0
                uv = pixels(cam, pos).astype(np.float64)
            ok &= np.isfinite(uv).all(axis=1)
            dense_joints[f, s] = int(ok.sum())
            if ok.sum() < p['min_joints']:
                continue
            sigma = np.minimum(np.sqrt(var), p['max_sigma'])
            mg = p['n_sigma'] * sigma * focal / pos[:, 2]
            lo = (uv - mg[:, None])[ok].min(axis=0)
            hi = (uv + mg[:, None])[ok].max(axis=0)
            centre, half = (lo + hi) / 2, (hi - lo) / 2 * p['expand']
            lo, hi = centre - half, centre + half
            if p['clip']:
                lo, hi = np.maximum(lo, 0.0), np.minimum(hi, sizes[f].astype(np.float64))
            for side in hi - lo:
                closer('side_px', side - p['min_side'])
            if (hi - lo >= p['min_side']).all():
                dense[f, s] = [lo[0], lo[1], hi[0] - lo[0], hi[1] - lo[1]]

    rows = []                                                   # (box, frame, slot, id, detection, joints)
    for f in range(n_frames):
        for s in range(n_tracks):
            if not np.isnan(dense[f, s, 0]):
                rows.append((dense[f, s], f, s, int(ids[s]), -1, int(dense_joints[f, s])))
    n_predicted, suppressed, bad, bad_frame = len(rows), 0, 0, 0
    det = c.get('det_boxes')
    if det is not None:
        for k, (b, f) in enumerate(zip(np.asarray(det, np.float64).reshape(-1, 4), c['det_frame'])):
            if not 0 <= f < n_frames:
                bad_frame += 1
                continue
            if not np.isfinite(b).all() or b[2] <= 0 or b[3] <= 0:
                bad += 1
                continue
            ious = [overlap(_corners(b), _corners(dense[f, s])) for s in range(n_tracks) if not np.isnan(dense[f, s, 0])]
            for v in ious:
                closer('iou', v - p['iou_max'])
            if any(v >= p['iou_max'] for v in ious):
                suppressed += 1
                continue
            rows.append((b, int(f), -1, -1, k, -1))
    ints = lambda i: np.asarray([r[i] for r in rows], np.int32).reshape(-1)
    return dict(boxes=np.asarray([r[0] for r in rows], np.float64).reshape(-1, 4), frame=ints(1), slot=ints(2), id=ints(3),
                detection=ints(4), n_joints=ints(5), counts=np.asarray([len(rows), n_predicted, suppressed, bad, bad_frame], np.int32),
                dense_boxes=dense, dense_joints=dense_joints, margins=margins)


def check_margins(c, want):
    """Every decision of the case is far enough from flipping that neither the comparison's tolerance nor a last bit changes it."""
    m = want['margins']
    assert np.asarray(c['sizes']).max() <= LIMIT_PX, 'the bound is worked out for frames up to 4096 px'
    assert m['near_mm'] >= MARGIN_MM and m['slope'] >= MARGIN_SLOPE and m['side_px'] >= MARGIN_PX, m
    assert m['iou'] >= MARGIN_IOU and m['age_s'] >= MARGIN_AGE_S, m


def compare(got, want):
    """Asserts: counts, joint counts, row order and every integer column exact, the NaN pattern of the dense boxes exact, box
    coordinates within BOX_PX.  -> the worst box deviation in pixels."""
    assert np.array_equal(got['counts'], want['counts']), (got['counts'], want['counts'])
    assert np.array_equal(got['dense_joints'], want['dense_joints'])
    assert np.array_equal(np.isnan(got['dense_boxes']), np.isnan(want['dense_boxes']))
    for key in ('frame', 'slot', 'id', 'detection', 'n_joints'):
        assert got[key].dtype == np.int32 and np.array_equal(got[key], want[key]), key
    worst = 0.0
    for key in ('dense_boxes', 'boxes'):
        g, w = got[key], want[key]
        assert g.dtype == np.float64 and g.shape == w.shape
        fin = ~np.isnan(w)
        if fin.any():
            worst = max(worst, float(np.abs(g[fin] - w[fin]).max()))
    assert worst <= BOX_PX, worst
    det = want['detection'] >= 0
    assert np.array_equal(got['boxes'][det], want['boxes'][det]), 'a detection comes out as it went in'
    return worst


# ---- cases -------------------------------------------------------------------------------------------------------------------

def pinhole(f=1000.0, w=1280, h=720, **kw):
    return Camera(np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1.0]]), **kw)


DISTORTION = (-0.25, 0.08, 0.001, -0.0005, -0.01)


def body(nj, seed=0):
    """Joint offsets [nj, 3] mm of a standing person 1.7 m tall and 0.5 m wide (y points down, like the image), fp32-exact."""
    rng = np.random.default_rng(seed)
    b = rng.uniform(-1, 1, (nj, 3)) * np.array([250.0, 850.0, 100.0])
    if nj >= 4:
        b[0], b[1], b[2], b[3] = (0, -850, 0), (0, 850, 0), (-250, 0, 0), (250, 0, 0)
    return np.round(b)


def joint_cov(sigma_p=20.0, sigma_v=300.0, rho=0.3):
    """A positive definite 6x6 P: isotropic position and velocity blocks, correlated."""
    i3 = np.eye(3)
    return np.block([[sigma_p ** 2 * i3, rho * sigma_p * sigma_v * i3], [rho * sigma_p * sigma_v * i3, sigma_v ** 2 * i3]])


def table(n_tracks, nj):
    state = np.zeros((n_tracks, nj, 28))
    state[..., 27] = np.nan
    return state, np.full(n_tracks, -1, np.int32)


def put(state, ids, slot, track_id, joints, velocity=(0, 0, 0), t_last=0.0, p=None):
    p = joint_cov() if p is None else p
    for j, x in enumerate(joints):
        state[slot, j] = TS.pack_state(np.concatenate([x, velocity]), p, t_last)
    ids[slot] = track_id


def case_standing():
    """A pinhole camera and a standing person 4 m in front of it, moving at 1.2 m/s to the right; defaults."""
    state, ids = table(3, 17)
    put(state, ids, 1, 5, body(17) + [200.0, 0, 4000.0], velocity=(1200.0, 0, 0))
    return dict(state=state, ids=ids, cameras=[pinhole()], sizes=[[1280, 720]], times=[0.1], coords='camera')


def case_tight():
    """expand = 1, n_sigma = 0: the box is the bounding box of the projections."""
    return dict(case_standing(), params=dict(expand=1.0, n_sigma=0.0))


def case_no_box():
    """Slot 0 free; 1 older than max_age_s; 2 behind the camera; 3 with fewer than min_joints joints in front of it; 4 wholly to the
    left of the frame; 5 across the left border (clipped); 6 a person whose id says free although it holds a state; 7 fine."""
    state, ids = table(8, 17)
    b = body(17)
    put(state, ids, 1, 11, b + [0, 0, 4000.0], t_last=-1.5)
    put(state, ids, 2, 12, b + [0, 0, -4000.0])
    front = b + [0, 0, 4000.0]
    front[5:, 2] = 50.0                                       # 12 joints nearer than near_mm: 5 visible < 9
    put(state, ids, 3, 13, front)
    put(state, ids, 4, 14, b + [-6000.0, 0, 4000.0])
    put(state, ids, 5, 15, b + [-2560.0, 0, 4000.0])
    put(state, ids, 6, 16, b + [600.0, 0, 4000.0])
    ids[6] = -1
    put(state, ids, 7, 17, b + [900.0, 0, 4000.0])
    return dict(state=state, ids=ids, cameras=[pinhole()], sizes=[[1280, 720]], times=[0.1], coords='camera')


def case_growth():
    """One still person, frames at growing dt: the margin grows with dt until sigma reaches max_sigma_mm."""
    state, ids = table(1, 17)
    put(state, ids, 0, 0, body(17) + [0, 0, 5000.0], p=joint_cov(10.0, 100.0, 0.0))
    times = [0.0, 0.05, 0.1, 0.2, 0.4, 0.8, 0.9, 0.95]
    return dict(state=state, ids=ids, cameras=[pinhole(w=4096, h=4096)], sizes=[[4096, 4096]] * len(times), times=times,
                coords='camera', params=dict(expand=1.0, clip=False))


def case_fold():
    """k1 < 0 alone: joint 1 lies beyond the monotonic range of the lens model (1 + 3 k1 r2 < 0) and its folded-back pixel is
    inside the frame; it is skipped.  min_joints 1."""
    cam = pinhole(distortion_coeffs=(-0.3, 0, 0, 0, 0))
    joints = np.array([[0, 0, 4000.0], [6400.0, 0, 4000.0], [300.0, 200.0, 4000.0], [-300.0, -200.0, 4000.0]])
    state, ids = table(1, 4)
    put(state, ids, 0, 0, joints)
    return dict(state=state, ids=ids, cameras=[cam], sizes=[[1280, 720]], times=[0.0], coords='camera',
                params=dict(expand=1.0, n_sigma=0.0, min_joints=1))


def rig():
    """Three distorted cameras on a 4 m circle, 1.5 m up, looking at a point 0.9 m above the origin of a z-up world."""
    cams = []
    for az in (0.0, 2.1, 4.2):
        centre = np.array([4000 * np.cos(az), 4000 * np.sin(az), 1500.0])
        z = (np.array([0, 0, 900.0]) - centre) / np.linalg.norm(np.array([0, 0, 900.0]) - centre)
        x = np.cross(z, [0, 0, 1.0])
        x /= np.linalg.norm(x)
        cams.append(pinhole(distortion_coeffs=DISTORTION, R=np.stack([x, np.cross(z, x), z]), t=centre))
    return cams


def world_body(nj, seed=0):
    b = body(nj, seed)
    return np.stack([b[:, 0], b[:, 2], -b[:, 1] + 900.0], axis=1)       # upright in a z-up world, feet near the floor


def case_world_rig():
    """World coordinates on the 3-camera rig: one slot gives one box per camera."""
    state, ids = table(2, 17)
    put(state, ids, 1, 3, world_body(17) + [200.0, -100.0, 0], velocity=(500.0, 300.0, 0))
    return dict(state=state, ids=ids, cameras=rig(), sizes=[[1280, 720]] * 3, times=[0.1] * 3, coords='world')


def case_camera_ignores_rt():
    """The rig's cameras with coords 'camera': R and t are not read, the state is in each frame's camera already."""
    state, ids = table(2, 17)
    put(state, ids, 0, 0, body(17) + [0, 0, 4500.0])
    return dict(state=state, ids=ids, cameras=rig(), sizes=[[1280, 720]] * 3, times=[0.1] * 3, coords='camera')


def _shifted(box, frac):
    return [box[0] + frac * box[2], box[1], box[2], box[3]]


def case_detections():
    """Two persons on frame 0 and the same two on frame 1 (the second one out of view there); detections: one just above and one
    just below iou_max against person 0, one on frame 1 where only frame 0 has the overlapping box (kept), a NaN one, a w = 0
    one, one far from everybody."""
    state, ids = table(4, 17)
    put(state, ids, 0, 7, body(17) + [-800.0, 0, 4000.0])
    put(state, ids, 2, 9, body(17, 1) + [2000.0, 0, 4000.0])
    c = dict(state=state, ids=ids, cameras=[pinhole(), pinhole(f=1000.0, w=640, h=720)], sizes=[[1280, 720], [640, 720]],
             times=[0.1, 0.1], coords='camera')
    b = predict(c)['dense_boxes']
    assert not np.isnan(b[0, 0, 0]) and not np.isnan(b[0, 2, 0]) and np.isnan(b[1, 2, 0])
    # two equal boxes shifted by a share d of their width overlap with IoU (1 - d) / (1 + d): 0.3 at d = 7 / 13
    above, below = _shifted(b[0, 0], 7 / 13 - 0.03), _shifted(b[0, 0], 7 / 13 + 0.03)
    other_frame = list(b[0, 2])                               # person 2's box of frame 0, given as a detection of frame 1
    det = [below, [10.0, 10.0, np.nan, 50.0], above, other_frame, [100.0, 100.0, 0.0, 80.0], [1100.0, 20.0, 60.0, 90.0]]
    return dict(c, det_boxes=np.asarray(det), det_frame=np.asarray([0, 0, 0, 1, 0, 0], np.int32))


def case_bad_frames():
    """The detections case with two frame indices outside [0, F): dropped, counted in the status word."""
    c = case_detections()
    return dict(c, det_frame=np.asarray([0, 0, 0, 2, -1, 0], np.int32))


def crowd(n_frames, n_tracks, nj, m, seed, all_present=False, none_present=False, distorted=True):
    """A table of n_tracks slots seen by n_frames cameras: most slots hold a person somewhere in a 10 m wide hall, some are
    free, some too old, some behind the camera, some with joints that have no state; m detections drawn from the predicted boxes
    (shifted a little, shifted a lot), from empty places and from invalid boxes.  Candidates whose overlap with some predicted
    box lies within 0.02 of iou_max are not taken (the restatement decides), so every case keeps its margin."""
    rng = np.random.default_rng(seed)
    state, ids = table(n_tracks, nj)
    for s in range(n_tracks):
        kind = 'person' if all_present else 'free' if none_present and s % 2 else 'behind' if none_present else \
            rng.choice(['person'] * 7 + ['free', 'old', 'behind'])
        if kind == 'free':
            continue
        centre = np.array([rng.uniform(-2500, 2500), rng.uniform(-300, 300), rng.uniform(3000, 7000)])
        if kind == 'behind':
            centre[2] = -centre[2]
        vel = rng.uniform(-1500, 1500, 3) * [1, 0.2, 1]
        put(state, ids, s, 100 + s, body(nj, seed + s) + np.round(centre), velocity=np.round(vel), t_last=-2.0 if kind == 'old' else 0.0,
            p=joint_cov(rng.uniform(5, 40), rng.uniform(50, 600), rng.uniform(-0.5, 0.5)))
        if kind == 'person' and not all_present and nj > 4 and rng.random() < 0.3:
            state[s, rng.integers(0, nj), 27] = np.nan        # a joint never seen
            state[s, rng.integers(0, nj), 27] = -0.05          # a joint seen earlier than the rest
    cams = [pinhole(f=float(rng.choice([800, 1000, 1400])), w=1280 + 64 * (f % 3), h=720 + 8 * (f % 2),
                    distortion_coeffs=DISTORTION if distorted and f % 2 == 0 else None) for f in range(n_frames)]
    sizes = [[1280 + 64 * (f % 3), 720 + 8 * (f % 2)] for f in range(n_frames)]
    times = [np.round(0.04 + 0.01 * (f % 5), 2) for f in range(n_frames)]
    c = dict(state=state, ids=ids, cameras=cams, sizes=sizes, times=times, coords='camera')
    if m == 0:
        return c
    want = predict(c)
    present = np.argwhere(~np.isnan(want['dense_boxes'][..., 0]))
    det, det_frame = [], []
    while len(det) < m:
        kind = rng.choice(['near', 'far', 'empty', 'bad']) if len(present) else rng.choice(['empty', 'bad'])
        f = int(rng.integers(0, n_frames))
        if kind in ('near', 'far'):
            f, s = present[rng.integers(0, len(present))]
            box = np.array(_shifted(want['dense_boxes'][f, s], rng.uniform(0.02, 0.2) if kind == 'near' else rng.uniform(0.7, 1.5)))
        elif kind == 'empty':
            box = np.array([rng.uniform(0, 1200), rng.uniform(0, 600), rng.uniform(20, 200), rng.uniform(40, 400)])
        else:
            box = np.array([100.0, 100.0, 50.0, 50.0])
            box[rng.integers(0, 4)] = rng.choice([np.nan, np.inf, 0.0, -5.0])
            if np.isfinite(box).all() and (box[2:] > 0).all():
                continue
        if np.isfinite(box).all() and (box[2:] > 0).all():
            ious = [overlap(_corners(box), _corners(b)) for b in want['dense_boxes'][f] if not np.isnan(b[0])]
            if any(abs(v - 0.3) < 0.02 for v in ious):
                continue
        det.append(box)
        det_frame.append(int(f))
    return dict(c, det_boxes=np.asarray(det), det_frame=np.asarray(det_frame, np.int32))


# name -> builder.  F T = 257 is prime and beyond both T <= 128 and F <= 64, so no table has it: 258 = 6 x 43 is the smallest
# size past the 256-row chunk of the compaction that a table can have.
CASES = {
    'standing': case_standing, 'tight': case_tight, 'no-box': case_no_box, 'growth': case_growth, 'fold': case_fold,
    'world-rig': case_world_rig, 'camera-ignores-rt': case_camera_ignores_rt, 'detections': case_detections,
    'bad-frames': case_bad_frames,
    'ft1-j1': lambda: crowd(1, 1, 1, 0, 1, all_present=True),
    'ft63-m1': lambda: crowd(1, 63, 17, 1, 2),
    'ft64-f64-m255': lambda: crowd(64, 1, 17, 255, 3, all_present=True),
    'ft64-t64': lambda: crowd(1, 64, 17, 0, 4),
    'ft65-m257': lambda: crowd(5, 13, 17, 257, 5),
    'ft255': lambda: crowd(3, 85, 17, 1, 6),
    'ft256-t128-all': lambda: crowd(2, 128, 17, 255, 7, all_present=True),
    'ft258': lambda: crowd(6, 43, 17, 257, 8),
    'ft513-all': lambda: crowd(27, 19, 17, 0, 9, all_present=True),
    'ft513': lambda: crowd(27, 19, 17, 257, 10),
    'none-present': lambda: crowd(3, 20, 17, 257, 11, none_present=True),
    'j64': lambda: crowd(2, 5, 64, 1, 12),
}


@functools.lru_cache(maxsize=None)
def case_and_expected(name):
    """(case, expected) computed once and shared by the tests of a session: treat both as read-only."""
    c = CASES[name]()
    return c, predict(c)
