"""fp64 NumPy restatement of metro_smooth_tracks, written from the header comment of include/metro_hip.h: the yardstick of
tests/test_track_smoothing.py (kernel code compiled for the host) and tests/test_gpu_track_smoothing.py (the launch).  Nothing
in the reference to compare with: one example is one image.  Deliberately unlike the kernel: dense 6x6 matrices, H, F and Q
written out, np.linalg.solve / inv / eigvalsh / cholesky where the kernel has cofactors, leading minors, a packed upper
triangle and an unpivoted LDL^T.  Also the test cases both files run."""
import functools

import numpy as np

MODES = ('filter', 'smooth')
MEASUREMENTS = ('isotropic', 'covariance')
J = 17
# bounds of the comparison (kernel vs this file rounded to fp32): one fp32 rounding below 8192 is <= 4.9e-4, and both sides
# compute in fp64 from the same fp32 inputs, so they differ by at most that one rounding step plus fp64 noise
POSITION_MM, VELOCITY_MM_S, COVARIANCE_REL, LIMIT = 1e-3, 1e-3, 1e-6, 8192.0
SENTINEL = -7.0
H = np.hstack([np.eye(3), np.zeros((3, 3))])


def measurement_noise(cov9, measurement, r_floor, cov_scale):
    """R of one (row, joint): fp64 3x3 from the row's fp32 covariance (its upper triangle, mirrored)."""
    if measurement == 'isotropic':
        return r_floor ** 2 * np.eye(3)
    c = np.asarray(cov9, np.float64).reshape(3, 3)
    c = np.triu(c) + np.triu(c, 1).T
    return cov_scale * c + r_floor ** 2 * np.eye(3)


def _usable(z, r):
    if not np.isfinite(z).all() or not np.isfinite(r).all():
        return False
    return bool(np.linalg.eigvalsh(r).min() > 0)


def _transition(dt, q):
    i3 = np.eye(3)
    f = np.block([[i3, dt * i3], [np.zeros((3, 3)), i3]])
    qm = q * np.block([[dt ** 3 / 3 * i3, dt ** 2 / 2 * i3], [dt ** 2 / 2 * i3, dt * i3]])
    return f, qm


def _step_dt(t, t_prev):
    dt = t - t_prev
    return dt if dt > 0 else 0.0


def unpack_state(s28):
    p = np.zeros((6, 6))
    p[np.triu_indices(6)] = s28[6:27]
    return s28[:6].copy(), p + np.triu(p, 1).T, s28[27]


def pack_state(x, p, t):
    return np.concatenate([x, p[np.triu_indices(6)], [t]])


def smooth_tracks(poses, cov, times, rows, starts, mode='smooth', measurement='covariance', q=4e6, r_floor=1.0, cov_scale=1.0,
                  v0=2000.0, gate=0.0, state=None, fill=SENTINEL):
    """-> (poses [n, J, 3], velocity [n, J, 3], covariance [n, J, 9], used uint8 [n, J], state or None), the float outputs in
    fp64 (the callers round), rows listed in no group left at `fill`."""
    poses = np.asarray(poses)
    n, nj = poses.shape[:2]
    n_tracks = len(starts) - 1
    out_p, out_v, out_c = (np.full((n, nj, k), float(fill)) for k in (3, 3, 9))
    used = np.full((n, nj), np.uint8(int(abs(fill))), np.uint8)
    state = None if state is None else np.array(state, np.float64)
    for tr in range(n_tracks):
        lo, hi = max(int(starts[tr]), 0), min(int(starts[tr + 1]), len(rows))
        listed = [int(r) for r in rows[lo:hi] if 0 <= int(r) < n]
        for j in range(nj):
            x = p = t_prev = None
            if state is not None and not np.isnan(state[tr, j, 27]):
                x, p, t_prev = unpack_state(state[tr, j])
            hist = []                                           # (row, x, P, x-, P-, F) of the rows with a state
            for row in listed:
                z = poses[row, j].astype(np.float64)
                r = measurement_noise(None if cov is None else cov[row, j], measurement, r_floor, cov_scale)
                ok = _usable(z, r)
                t = float(times[row])
                if x is None:
                    if not ok:
                        out_p[row, j], out_v[row, j], out_c[row, j], used[row, j] = np.nan, np.nan, np.nan, 0
                        continue
                    x = np.concatenate([z, np.zeros(3)])
                    p = np.zeros((6, 6))
                    p[:3, :3], p[3:, 3:] = r, v0 ** 2 * np.eye(3)
                    hist.append((row, x, p, x, p, np.eye(6)))
                    used[row, j], t_prev = 1, t
                    continue
                f, qm = _transition(_step_dt(t, t_prev), q)
                xm, pm = f @ x, f @ p @ f.T + qm
                x, p, u = xm, pm, 0
                if ok:
                    nu = z - H @ xm
                    s = H @ pm @ H.T + r
                    if not (gate > 0 and nu @ np.linalg.solve(s, nu) > gate):
                        k = pm @ H.T @ np.linalg.inv(s)
                        a = np.eye(6) - k @ H
                        x, p, u = xm + k @ nu, a @ pm @ a.T + k @ r @ k.T, 1
                hist.append((row, x, p, xm, pm, f))
                used[row, j], t_prev = u, t
            if not hist:
                continue
            if state is not None:
                state[tr, j] = pack_state(hist[-1][1], hist[-1][2], t_prev)
            xs, ps = hist[-1][1], hist[-1][2]
            res = {len(hist) - 1: (xs, ps)}
            for i in range(len(hist) - 2, -1, -1):
                _, xf, pf, _, _, _ = hist[i]
                _, _, _, xm1, pm1, f1 = hist[i + 1]
                if mode == 'smooth' and _positive_definite(pm1):
                    c = np.linalg.solve(pm1, f1 @ pf).T               # P_k F^T P-^-1, both P symmetric
                    xs, ps = xf + c @ (xs - xm1), pf + c @ (ps - pm1) @ c.T
                else:
                    xs, ps = xf, pf
                res[i] = (xs, ps)
            for i, (row, *_rest) in enumerate(hist):
                out_p[row, j], out_v[row, j], out_c[row, j] = res[i][0][:3], res[i][0][3:], res[i][1][:3, :3].reshape(9)
    return out_p, out_v, out_c, used, state


def _positive_definite(p):
    try:
        np.linalg.cholesky(p)
        return True
    except np.linalg.LinAlgError:
        return False


def alpha_beta_gain(q, dt, sigma):
    """The steady-state position gain alpha of a constant-velocity filter with white-noise acceleration of density q,
    sampled every dt with position noise sigma.  With lam^2 = q dt^3 / sigma^2 the steady-state Riccati equations reduce to
    beta^2 / (1 - alpha) = lam^2 and alpha^2 = (2 - alpha) beta - beta^2 / 6; with x = sqrt(1 - alpha) that is the
    palindromic quartic x^4 - lam x^3 + (lam^2/6 - 2) x^2 - lam x + 1 = 0, solved through y = x + 1/x."""
    lam = np.sqrt(q * dt ** 3) / sigma
    y = (lam + np.sqrt(lam ** 2 / 3 + 16)) / 2
    x = (y - np.sqrt(y ** 2 - 4)) / 2
    return 1 - x ** 2


# ---- cases -------------------------------------------------------------------------------------------------------------------

def _motion(rng, t, nj):
    """Smooth joint tracks [T, nj, 3] mm inside 8 m: a person swaying at 2 - 4 m depth."""
    phase = rng.uniform(0, 2 * np.pi, (1, nj, 3))
    amp = rng.uniform(50, 300, (1, nj, 3))
    centre = np.array([0.0, 0.0, 3000.0]) + rng.uniform(-800, 800, (1, nj, 3))
    return centre + amp * np.sin(2 * np.pi * 0.5 * t[:, None, None] + phase) + 200.0 * t[:, None, None] * np.array([1.0, 0.2, -0.5])


def _random_cov(rng, shape, sigma=(5.0, 20.0)):
    """Symmetric positive definite 3x3 mm^2, fp32 [*shape, 9]."""
    a = rng.normal(size=shape + (3, 3))
    q, _ = np.linalg.qr(a)
    s = rng.uniform(*sigma, shape + (3,)) ** 2
    c = np.einsum('...ij,...j,...kj->...ik', q, s, q)
    c = (c + np.swapaxes(c, -1, -2)) / 2
    return c.reshape(shape + (9,)).astype(np.float32)


def build(lengths, seed, mode, measurement, nj=J, extra_rows=2, fps=30.0, gate=0.0, sigma=10.0):
    """Tracks of the given lengths whose rows are scattered over memory, plus `extra_rows` rows in no group."""
    rng = np.random.default_rng(seed)
    n = int(sum(lengths)) + extra_rows
    where = rng.permutation(n)                       # memory row of the k-th generated row
    poses = rng.uniform(-100, 100, (n, nj, 3)).astype(np.float32)
    cov = _random_cov(rng, (n, nj))
    times = rng.uniform(0, 1, n)
    rows, starts, at = [], [0], 0
    for length in lengths:
        t = 0.25 + np.cumsum(rng.uniform(0.7, 1.3, length)) / fps          # uneven frame times
        mine = where[at:at + length]
        truth = _motion(rng, t, nj)
        noise = rng.normal(size=truth.shape) * sigma
        if measurement == 'covariance':                # noise with the covariance the row declares
            noise = np.einsum('...ik,...k->...i', np.linalg.cholesky(cov[mine].reshape(length, nj, 3, 3).astype(np.float64)), noise / sigma)
        poses[mine] = (truth + noise).astype(np.float32)
        times[mine] = t
        rows += list(mine)
        starts.append(len(rows))
        at += length
    return dict(poses=poses, cov=cov, times=times, rows=np.asarray(rows, np.int32), starts=np.asarray(starts, np.int32), mode=mode,
                measurement=measurement, q=4e6, r_floor=1.0 if measurement == 'covariance' else sigma, cov_scale=1.0, v0=2000.0,
                gate=gate)


def _track_rows(c, tr):
    return c['rows'][c['starts'][tr]:c['starts'][tr + 1]]


def case_ragged(mode, measurement):
    """Lengths 1, 2, 3 and 65, rows scrambled in memory, two rows in no group."""
    return build([1, 2, 3, 65], 11, mode, measurement)


def case_gaps(mode, measurement):
    """Track 0: NaN poses in the middle (rows 5-7), one joint with a lone NaN component; track 1: NaN rows at its start (0, 1) and
    one joint that starts a row later still; track 2: a covariance row that is not positive definite, and one with a NaN."""
    c = build([12, 9, 8], 12, mode, measurement)
    r0, r1, r2 = (_track_rows(c, k) for k in range(3))
    c['poses'][r0[5:8]] = np.nan
    c['poses'][r0[9], 3, 1] = np.inf
    c['poses'][r1[:2]] = np.nan
    c['poses'][r1[2], 4, 2] = np.nan
    c['cov'][r2[3], :, :] = np.float32([100, 0, 0, 0, -50, 0, 0, 0, 100])
    c['cov'][r2[5], 2, 4] = np.nan
    c['cov'][r2[0], 6] = np.float32([100, 150, 0, 0, 100, 0, 0, 0, 100])      # xy > sqrt(xx yy): indefinite at the first row
    return c


def case_skipped(mode, measurement):
    """Row indices outside [0, n) inside a group (skipped as if not listed), an empty group, a group holding only such
    indices, and group offsets beyond [0, n_rows] (clamped)."""
    c = build([6, 5], 13, mode, measurement)
    n = len(c['poses'])
    r0, r1 = _track_rows(c, 0), _track_rows(c, 1)
    rows = list(r0[:3]) + [-1, n + 5] + list(r0[3:]) + [n, -3] + list(r1)
    c['rows'] = np.asarray(rows, np.int32)
    c['starts'] = np.asarray([-2, 8, 8, 10, 15 + 9], np.int32)       # track 0, empty, out-of-range only, track 1 (clamped to 15)
    return c


def case_gated(mode, measurement):
    """gate = 25 with a 400 mm outlier on row 10 of track 0 (all joints) and on one joint of row 4 of track 1."""
    c = build([20, 8], 14, mode, measurement, gate=25.0)
    c['poses'][_track_rows(c, 0)[10]] += np.float32(400.0)
    c['poses'][_track_rows(c, 1)[4], 7, 0] -= np.float32(400.0)
    return c


def case_threads255(mode, measurement):
    """15 tracks x 17 joints = 255 threads: one block, its last lane idle."""
    return build([4] * 15, 15, mode, measurement, extra_rows=1)


def case_threads272(mode, measurement):
    """16 tracks x 17 joints = 272 threads: across the 256-thread block."""
    return build([4] * 16, 16, mode, measurement, extra_rows=1)


CASES = {'ragged': case_ragged, 'gaps': case_gaps, 'skipped': case_skipped, 'gated': case_gated, 'threads255': case_threads255,
         'threads272': case_threads272}


@functools.lru_cache(maxsize=None)
def case_and_expected(name, mode, measurement):
    """(case, expected) computed once and shared by the tests of a session: treat both as read-only."""
    c = CASES[name](mode, measurement)
    return c, expected(c)


def run_ref(c, state=None, **changes):
    a = {**c, **changes}
    return smooth_tracks(a['poses'], a['cov'], a['times'], a['rows'], a['starts'], a['mode'], a['measurement'], a['q'], a['r_floor'],
                         a['cov_scale'], a['v0'], a['gate'], state)


def expected(c, state=None):
    """The restatement rounded once to fp32, as the kernel rounds: (poses, velocity, covariance, used)."""
    p, v, cv, used, _ = run_ref(c, state)
    with np.errstate(invalid='ignore'):
        return p.astype(np.float32), v.astype(np.float32), cv.astype(np.float32), used


def compare(got, want):
    """Asserts the bounds of the issue; -> the worst deviations (mm, mm/s, relative to the covariance block's largest entry)."""
    worst = []
    for g, w, bound in zip(got[:2], want[:2], (POSITION_MM, VELOCITY_MM_S)):
        assert g.dtype == np.float32 and g.shape == w.shape
        assert np.array_equal(np.isnan(g), np.isnan(w)), 'NaN pattern'
        fin = ~np.isnan(w)
        assert np.abs(w[fin]).max() < LIMIT, 'the cases stay inside the range the bound is worked out for'
        dev = np.abs(g[fin].astype(np.float64) - w[fin]).max()
        worst.append(dev)
        assert dev <= bound, (dev, bound)
    g, w = got[2].astype(np.float64), want[2].astype(np.float64)
    assert got[2].dtype == np.float32 and np.array_equal(np.isnan(g), np.isnan(w)), 'covariance NaN pattern'
    fin = ~np.isnan(w).any(axis=-1)
    rel = (np.abs(g - w)[fin] / np.abs(w[fin]).max(axis=-1, keepdims=True)).max()
    worst.append(rel)
    assert rel <= COVARIANCE_REL, rel
    assert got[3].dtype == np.uint8 and np.array_equal(got[3], want[3]), 'used'
    return worst


def check_case(name, c, got):
    """What each case is there to show, on the outputs of whoever ran it."""
    poses, vel, cov, used = got
    listed = np.zeros(len(c['poses']), bool)
    for tr in range(len(c['starts']) - 1):
        r = c['rows'][max(c['starts'][tr], 0):min(c['starts'][tr + 1], len(c['rows']))]
        listed[r[(r >= 0) & (r < len(listed))]] = True
    assert (~listed).any() and (poses[~listed] == SENTINEL).all() and (vel[~listed] == SENTINEL).all()
    assert (cov[~listed] == SENTINEL).all() and (used[~listed] == int(abs(SENTINEL))).all(), 'rows in no group are not written'
    assert (used[listed] <= 1).all() and not (poses[listed] == SENTINEL).any()
    covariance = c['measurement'] == 'covariance'
    if name == 'ragged':
        one = _track_rows(c, 0)[0]
        assert np.array_equal(poses[one], c['poses'][one]) and (vel[one] == 0).all() and used[one].all()     # a one-row track: its input
    if name == 'gaps':
        r0, r1, r2 = (_track_rows(c, k) for k in range(3))
        assert not used[r0[5:8]].any() and np.isfinite(poses[r0[5:8]]).all(), 'a gap is bridged by the prediction'
        assert used[r0[9], 3] == 0 and used[r0[9]].sum() == J - 1
        assert np.isnan(poses[r1[:2]]).all() and np.isnan(vel[r1[:2]]).all() and np.isnan(cov[r1[:2]]).all() and not used[r1[:2]].any()
        assert np.isnan(poses[r1[2], 4]).all() and np.isfinite(np.delete(poses[r1[2]], 4, axis=0)).all() and used[r1[3]].all()
        assert used[r2[3]].any() != covariance and (used[r2[5], 2] == 0) == covariance
        assert np.isnan(poses[r2[0], 6]).all() == covariance
    if name == 'skipped':
        assert used[c['rows'][[0, 1, 2, 5, 6, 7]]].all() and used[c['rows'][10:15]].all()
    if name == 'gated':
        r0, r1 = _track_rows(c, 0), _track_rows(c, 1)
        assert not used[r0[10]].any() and used[r0[9]].all() and used[r0[11]].all()
        assert used[r1[4], 7] == 0 and used[r1[4]].sum() == J - 1
