"""fp64 NumPy restatement of the track-predicted heat-map prior (metro_plan_bind_track_prior, include/metro_hip.h), written
unlike the kernel: the slots are a Python dict, the prediction is the dense 6 x 6 F P F^T + Q, K and Sigma are inverted by
np.linalg.inv, the projection Jacobian is a dense matrix product (tests/test_track_prior.py checks it once against central
differences), and every row is a walk through plain arrays.  Also what the tests share: the case builder, the margins that keep
every compared case away from a decision the tolerance could flip, and the bounds of the issue."""
import numpy as np

from metro_pose3d_amd import _lib

STATE = 28
GIVEN, NO_SLOT, NO_STATE, TOO_OLD, NEAR, SINGULAR, NONFINITE = range(7)
PLACEMENT = np.dtype(_lib.MetroPlacement)
DEFAULTS = dict(accel_psd=4e6, max_age_s=1.0, near_mm=100.0, sigma_floor_mm=30.0, cov_scale=1.0)

# the bounds the tests hold (both sides compute in fp64 and round once to fp32)
MU_BOUND = 2.4e-7               # |mu - ref| <= MU_BOUND max(1, |ref|): two fp32 roundings of values that agree to 1e-13
BLOCK_BOUND = 1e-6              # each precision block within this of its largest entry: the bound of fp32-rounded matrix blocks
AGE_MARGIN_S, NEAR_MARGIN_MM, MAX_COND = 1e-3, 1e-1, 1e4


class Head:
    """What the prior needs of a model's head: heatmap_to_image's constants, the box size, the head joints and the output order."""

    def __init__(self, spec, n_out=None):
        """n_out: the first n_out joints of the output order only (a skeleton of one joint has no model of its own)."""
        last = spec.proc_side - 1
        self.lrc = float(last - last % spec.stride - 1)
        self.half = float(spec.stride // 2) if spec.centered_stride else 0.0
        self.box = float(spec.box_size_mm)
        self.side = int(spec.proc_side)
        self.n_head = spec.skeleton.n_head
        self.perm = list(spec.skeleton.permutation)[:n_out]
        self.mirror = [m if m < len(self.perm) else r for r, m in enumerate(list(spec.skeleton.out_mirror)[:n_out])]
        self.cspec = spec.to_c(1)
        self.cspec.n_joints_out = len(self.perm)
        self.n_out = len(self.perm)
        self.root_out = self.perm.index(self.n_head - 1) if self.n_head - 1 in self.perm else -1


def unpack_state(st):
    """st [28] -> (x [6], P [6, 6], t_last)."""
    p = np.zeros((6, 6))
    p[np.triu_indices(6)] = st[6:27]
    return st[:6].copy(), p + np.triu(p, 1).T, st[27]


def pack_state(x, p, t_last):
    return np.concatenate([x, np.asarray(p)[np.triu_indices(6)], [t_last]])


def predict_dense(x, p, dt, q):
    """The constant-velocity prediction as matrices: F x, F P F^T + Q."""
    i3, z3 = np.eye(3), np.zeros((3, 3))
    f = np.block([[i3, dt * i3], [z3, i3]])
    qm = q * np.block([[dt ** 3 / 3 * i3, dt ** 2 / 2 * i3], [dt ** 2 / 2 * i3, dt * i3]])
    return f @ x, f @ p @ f.T + qm


def project(c, k, head):
    """A point of the crop's virtual camera -> heat-map units (x, y): the inverse of heatmap_to_image on K (x/z, y/z, 1)."""
    uv = (k @ np.array([c[0] / c[2], c[1] / c[2], 1.0]))[:2]
    return (uv - head.half) / head.lrc


def jacobian(c, k, head):
    """d project / dc as a product of dense matrices: [2 x 2 of K] [d (x/z, y/z) / dc] / lrc."""
    x, y, z = c
    return k[:2, :2] @ np.array([[1 / z, 0, -x / z ** 2], [0, 1 / z, -y / z ** 2]]) / head.lrc


def _camera_point(table, s, src, t, rec, world, params):
    """-> (reason, c, C_c, age margin)."""
    x, p, t_last = unpack_state(table[s][src])
    if np.isnan(t_last):
        return NO_STATE, None, None, None
    if not np.isfinite(t):
        return NONFINITE, None, None, None
    age = t - t_last
    if age > params['max_age_s']:
        return TOO_OLD, None, None, abs(age - params['max_age_s'])
    xm, pm = predict_dense(x, p, max(age, 0.0), params['accel_psd'])
    cov = params['cov_scale'] * pm[:3, :3] + params['sigma_floor_mm'] ** 2 * np.eye(3)
    rot = np.asarray(rec['rot_to_world' if world else 'rot_to_orig_cam'], np.float64).reshape(3, 3)
    c = rot.T @ (xm[:3] - np.asarray(rec['cam_loc'], np.float64) if world else xm[:3])
    cc = rot.T @ cov @ rot
    if not np.isfinite(c).all():
        return NONFINITE, c, cc, abs(age - params['max_age_s'])
    return (NEAR if c[2] < params['near_mm'] else GIVEN), c, cc, abs(age - params['max_age_s'])


def prior(case):
    """case: dict(head, state [T, Jout, 28], slot [n], times [n], records PLACEMENT [n], coords 'camera' | 'world', depth 'none' |
    'root', params, coords01 [n, J_head, 3] (read with depth 'root')) -> (prior float32 [n, Jout, 9], reason int32 [n, Jout],
    margins dict(age [s], near [mm], cond: the smallest / largest of those any row's decision had))."""
    head, params, world = case['head'], dict(DEFAULTS, **case.get('params', {})), case['coords'] == 'world'
    table = {s: rows for s, rows in enumerate(np.asarray(case['state'], np.float64))}
    n = len(case['slot'])
    out = np.zeros((n, head.n_out, 9))
    why = np.zeros((n, head.n_out), np.int32)
    margins = dict(age=np.inf, near=np.inf, cond=0.0)

    def note(age=None, c=None):
        if age is not None:
            margins['age'] = min(margins['age'], age)
        if c is not None and np.isfinite(c[2]):
            margins['near'] = min(margins['near'], abs(c[2] - params['near_mm']))
    for i in range(n):
        s, t, rec = int(case['slot'][i]), float(case['times'][i]), case['records'][i]
        rot = np.asarray(rec['rot_to_world' if world else 'rot_to_orig_cam'], np.float64).reshape(3, 3)
        flipped = not np.linalg.det(rot) > 0
        for r in range(head.n_out):
            if s not in table:
                why[i, r] = NO_SLOT
                continue
            src = head.mirror[r] if flipped else r
            reason, c, cc, age = _camera_point(table, s, src, t, rec, world, params)
            note(age, c)
            if reason != GIVEN:
                why[i, r] = reason
                continue
            with np.errstate(all='ignore'):
                k = np.linalg.inv(np.asarray(rec['inv_intrinsics'], np.float64).reshape(3, 3))
                mu = project(c, k, head)
                jac = jacobian(c, k, head)
                sigma = jac @ cc @ jac.T
                det = sigma[0, 0] * sigma[1, 1] - sigma[0, 1] ** 2
            if not np.isfinite(mu).all():
                why[i, r] = NONFINITE
                continue
            if not (np.isfinite(det) and det > 0):
                why[i, r] = SINGULAR
                continue
            margins['cond'] = max(margins['cond'], np.linalg.cond(sigma))
            lxy = np.linalg.inv(sigma)
            out[i, r, :2] = mu
            out[i, r, [3, 4, 6]] = lxy[0, 0], lxy[1, 1], lxy[0, 1]
            if case['depth'] == 'root' and head.root_out >= 0 and r != head.root_out:
                src0 = head.mirror[head.root_out] if flipped else head.root_out
                reason0, c0, cc0, age0 = _camera_point(table, s, src0, t, rec, world, params)
                note(age0, c0)
                if reason0 == GIVEN:
                    out[i, r, 2] = float(np.float32(case['coords01'][i, head.n_head - 1, 2])) + (c[2] - c0[2]) / head.box
                    out[i, r, 5] = head.box ** 2 / (cc[2, 2] + cc0[2, 2])
    return out.astype(np.float32), why, margins


def check_margins(margins, what=''):
    """The allowed deviation cannot change a reason word: every decision of a compared case lies this far from its threshold."""
    assert margins['age'] >= AGE_MARGIN_S and margins['near'] >= NEAR_MARGIN_MM and margins['cond'] <= MAX_COND, (what, margins)


def deviation(got_prior, got_reason, ref_prior, ref_reason):
    """The reason words exactly; -> dict(mu: worst |mu - ref| / max(1, |ref|), block: worst deviation of a precision block over its
    largest entry; the xy block (xx, yy, xy) and the z word are blocks of their own)."""
    got_prior, ref_prior = np.asarray(got_prior, np.float64), np.asarray(ref_prior, np.float64)
    assert np.array_equal(np.asarray(got_reason), ref_reason), 'reason words'
    assert (got_prior[np.asarray(ref_reason) != GIVEN] == 0.0).all(), 'a row without a prior is nine zeros'
    mu = np.abs(got_prior[..., :3] - ref_prior[..., :3]) / np.maximum(1.0, np.abs(ref_prior[..., :3]))
    worst = 0.0
    for words in ([3, 4, 6], [5]):
        size = np.abs(ref_prior[..., words]).max(-1)
        err = np.abs(got_prior[..., words] - ref_prior[..., words]).max(-1)
        on = size > 0
        assert (err[~on] == 0.0).all(), 'a zero block stays zero'
        if on.any():
            worst = max(worst, float((err[on] / size[on]).max()))
    assert (got_prior[..., 7:] == 0.0).all(), 'the xz and yz words are zero'
    return dict(mu=float(mu.max()) if mu.size else 0.0, block=worst)


def check(got_prior, got_reason, ref_prior, ref_reason, what=''):
    dev = deviation(got_prior, got_reason, ref_prior, ref_reason)
    print(f'track_prior {what}: mu {dev["mu"]:.3e} (bound {MU_BOUND:.1e}) block {dev["block"]:.3e} (bound {BLOCK_BOUND:.1e})')
    assert dev['mu'] <= MU_BOUND and dev['block'] <= BLOCK_BOUND, (what, dev)
    return dev


# ---- cases -------------------------------------------------------------------------------------------------------------------

def rotation(rng, angle=0.4):
    """A proper rotation by at most `angle` rad about a random axis (Rodrigues)."""
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    a = rng.uniform(-angle, angle)
    kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * kx + (1 - np.cos(a)) * kx @ kx


def record(k, rot_to_world=None, orig_r=None, cam_loc=(0, 0, 0)):
    """One MetroPlacement with the fields the prior reads: inv(K), rot_to_world = virt.R^T, rot_to_orig_cam = orig.R virt.R^T."""
    rec = np.zeros((), PLACEMENT)
    rtw = np.eye(3) if rot_to_world is None else np.asarray(rot_to_world, np.float64)
    rec['inv_intrinsics'] = np.linalg.inv(np.asarray(k, np.float64)).astype(np.float32).reshape(-1)
    rec['rot_to_world'] = rtw.astype(np.float32).reshape(-1)
    rec['rot_to_orig_cam'] = ((np.eye(3) if orig_r is None else np.asarray(orig_r, np.float64)) @ rtw).astype(np.float32).reshape(-1)
    rec['cam_loc'] = np.asarray(cam_loc, np.float32)
    return rec


def pinhole(f=550.0, c=128.0):
    return np.array([[f, 0, c], [0, f, c], [0, 0, 1.0]])


def empty_state(n_tracks, n_out):
    state = np.zeros((n_tracks, n_out, STATE))
    state[..., 27] = np.nan
    return state


def random_cov6(rng, lo=25.0, hi=100.0, v_lo=200.0, v_hi=800.0):
    """A positive definite 6 x 6: position axes of lo..hi mm, velocity axes of v_lo..v_hi mm/s, weakly coupled."""
    scale = np.concatenate([rng.uniform(lo, hi, 3), rng.uniform(v_lo, v_hi, 3)])
    a = np.eye(6) + 0.15 * rng.standard_normal((6, 6))
    return (a @ a.T) * np.outer(scale, scale)


SPECIAL = ('slot -1', 'slot T', 'no state', 'too old', 'near', 'nan time')


def random_case(head, n, n_tracks, coords, depth, views=1, seed=0, params=None):
    """n crop rows (box-major with `views` views a box; the last view of a box is flipped when views > 1) over a table of n_tracks
    slots.  Rows cycle through the ordinary kind and, every seventh row on, the SPECIAL ones; joints sit 3 to 6 m in front of
    each row's virtual camera; times keep every decision AGE_MARGIN_S from max_age_s and NEAR_MARGIN_MM from near_mm."""
    rng = np.random.default_rng([seed, n, n_tracks, head.n_out, views, coords == 'world', depth == 'root'])
    p = dict(DEFAULTS, **(params or {}))
    world = coords == 'world'
    state = empty_state(n_tracks, head.n_out)
    t0 = 10.0
    for s in range(n_tracks):
        centre = np.array([rng.uniform(-400, 400), rng.uniform(-300, 300), rng.uniform(3500, 5500)])
        for r in range(head.n_out):
            x = np.concatenate([centre + rng.uniform(-450, 450, 3), rng.uniform(-1000, 1000, 3)])
            state[s, r] = pack_state(x, random_cov6(rng), t0 + 0.01 * (s % 3))
    orig_r = rotation(rng, 0.8) if world else np.eye(3)           # the original camera's R: world -> camera
    orig_t = rng.uniform(-2000, 2000, 3) if world else np.zeros(3)
    if world:                                                     # the table lives in the world: x_w = R^T x_c + t
        state[..., :3] = state[..., :3] @ orig_r + orig_t
        state[..., 3:6] = state[..., 3:6] @ orig_r
        big = np.zeros((6, 6))
        big[:3, :3] = big[3:, 3:] = orig_r.T
        for s in range(n_tracks):
            for r in range(head.n_out):
                x, pm, tl = unpack_state(state[s, r])
                state[s, r] = pack_state(x, big @ pm @ big.T, tl)
    slot, times, records, kinds = np.zeros(n, np.int32), np.zeros(n), np.zeros(n, PLACEMENT), []
    for i in range(n):
        box, view = divmod(i, views)
        s = box % n_tracks
        kind = SPECIAL[(box // 7) % len(SPECIAL)] if box % 7 == 6 else 'ordinary'
        kinds.append(kind)
        virt = rotation(rng, 0.25)                                # the virtual camera's turn away from the original's axis
        if views > 1 and view == views - 1:
            virt = virt @ np.diag([-1.0, 1.0, 1.0])               # a flipped view: det <= 0
        # virt maps crop-camera coordinates to the original camera's: rot_to_orig_cam = virt, rot_to_world = orig.R^T virt
        # a person of 1.8 m at 4.5 m fills the crop: f about 2.2 crop sides, the principal point at the crop's centre
        k = pinhole(head.side * rng.uniform(1.6, 2.7), head.side / 2 + rng.uniform(-3, 3))
        k[0, 1] = rng.uniform(-2, 2)
        rec = np.zeros((), PLACEMENT)
        rec['inv_intrinsics'] = np.linalg.inv(k).astype(np.float32).reshape(-1)
        rec['rot_to_orig_cam'] = virt.astype(np.float32).reshape(-1)
        rec['rot_to_world'] = (orig_r.T @ virt).astype(np.float32).reshape(-1)
        rec['cam_loc'] = orig_t.astype(np.float32)
        records[i] = rec
        slot[i] = s
        times[i] = t0 + 0.02 + (0.0, 0.04, 0.35, -0.5)[box % 4]
        if kind == 'slot -1':
            slot[i] = -1
        elif kind == 'slot T':
            slot[i] = n_tracks
        elif kind == 'too old':
            times[i] = t0 + 0.01 * (s % 3) + p['max_age_s'] + 0.01          # 10 ms past the age limit of its slot
        elif kind == 'nan time':
            times[i] = np.nan
    case = dict(head=head, state=state, slot=slot, times=times, records=records, coords=coords, depth=depth, params=p, kinds=kinds,
                coords01=rng.uniform(0.2, 0.8, (n, head.n_head, 3)).astype(np.float32))
    # 'no state' and 'near' act on the table: one joint of the row's slot each, restored for no other row (the rows that share the
    # slot see them too, which is the point: a joint without a state gives no prior wherever its slot is read)
    for i, kind in enumerate(kinds):
        if head.n_out == 1 and n_tracks == 1:
            break                                                   # one joint in one slot: every row would lose its prior
        if kind == 'no state' and i % views == 0:
            state[slot[i], (i // views) % head.n_out, 27] = np.nan
        if kind == 'near' and i % views == 0:
            r = (i // views) % head.n_out
            rot = np.asarray(records[i]['rot_to_world' if world else 'rot_to_orig_cam'], np.float64).reshape(3, 3)
            # on the axis of this row's camera at 0.6 near_mm: every camera of the case shares its centre and is turned by less
            # than 1 rad from this one, so the joint is nearer than near_mm to all of them, by more than the margin
            cam = np.array([0.0, 0.0, 0.6 * p['near_mm']])
            x, pm, tl = unpack_state(state[slot[i], r])
            x[:3] = rot @ cam + (np.asarray(records[i]['cam_loc'], np.float64) if world else 0.0)
            x[3:] = 0.0
            state[slot[i], r] = pack_state(x, pm, tl)
    return case
