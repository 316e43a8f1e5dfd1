"""fp64 NumPy restatement of metro_track_bone_lengths, written from the header comment of include/metro_hip.h and deliberately
unlike the kernel: it keeps no running sums.  A table is a dict of per-slot ids and, per (slot, edge), the LIST of the accepted
samples (l^, v); the mean is np.average over that list, u^T C u an np.einsum over dense 3x3 matrices computed for all rows of an
edge at once, and the gate is replayed against the list as it stood when the row arrived.  Also the cases both test files share."""
import numpy as np

DEFAULTS = dict(min_count=8, gate=9.0, sigma_floor_mm=1.0, cov_scale=1.0, min_length_mm=1.0, debias=True, symmetric=True)


def new_table(n_tracks, n_edges):
    return dict(ids=[-1] * n_tracks, samples={(t, e): [] for t in range(n_tracks) for e in range(n_edges)},
                rejected={(t, e): 0 for t in range(n_tracks) for e in range(n_edges)}, margins=[], T=n_tracks, E=n_edges)


def dense_cov(cov):
    """[n, J, 9] or [n, J, 3, 3] of which the upper triangle counts -> symmetric [n, J, 3, 3]."""
    c = np.asarray(cov, np.float64).reshape(len(cov), -1, 3, 3)
    upper = np.triu(c)
    return upper + np.swapaxes(np.triu(c, 1), -1, -2)


def samples_of(poses, cov, rows, a, b, sigma_floor_mm, cov_scale, min_length_mm, debias):
    """(l^, v) of the listed rows for the edge (a, b), in order; rows that the model skips are left out."""
    rows = np.asarray(rows, np.int64)
    if len(rows) == 0:
        return []
    p = np.asarray(poses, np.float64)
    d = p[rows, b] - p[rows, a]
    with np.errstate(all='ignore'):
        ok = np.isfinite(p[rows, a]).all(-1) & np.isfinite(p[rows, b]).all(-1)
        l = np.linalg.norm(d, axis=-1)
        ok &= l >= min_length_mm
        if cov is None:
            lh, v = l.copy(), np.full(len(rows), sigma_floor_mm ** 2)
        else:
            c = cov_scale * (cov[rows, a] + cov[rows, b])
            ok &= np.isfinite(c[:, np.triu_indices(3)[0], np.triu_indices(3)[1]]).all(-1)
            ok &= (np.diagonal(c, axis1=-2, axis2=-1) >= 0).all(-1)
            u = d / l[:, None]
            q = np.einsum('ri,rij,rj->r', u, c, u)
            tr = np.trace(c, axis1=-2, axis2=-1)
            v = tr / 3.0 + sigma_floor_mm ** 2
            lh = l - (tr - q) / (2.0 * l) if debias else l.copy()
        ok &= lh > 0
    return [(float(lh[k]), float(v[k])) for k in np.flatnonzero(ok)]


def update(table, poses, cov, rows, starts, ids, edges, min_count=8, gate=9.0, sigma_floor_mm=1.0, cov_scale=1.0, min_length_mm=1.0,
           debias=True, symmetric=True):
    """One launch's steps 0 and 1 on `table`, in place.  poses None: the reset alone."""
    del symmetric
    ids = [int(i) for i in ids]
    for t in range(table['T']):
        if table['ids'][t] != ids[t]:
            for e in range(table['E']):
                table['samples'][t, e], table['rejected'][t, e] = [], 0
            table['ids'][t] = ids[t]
    if poses is None or len(np.asarray(rows)) == 0:
        return table
    n, nj = np.asarray(poses).shape[:2]
    cov = None if cov is None else dense_cov(cov)
    rows, starts = np.asarray(rows, np.int64), np.clip(np.asarray(starts, np.int64), 0, len(np.asarray(rows)))
    for t in range(table['T']):
        mine = rows[starts[t]:starts[t + 1]]
        mine = mine[(mine >= 0) & (mine < n)]
        for e, (a, b) in enumerate(np.asarray(edges, np.int64).reshape(-1, 2)):
            if not (0 <= a < nj and 0 <= b < nj):
                continue
            kept = table['samples'][t, e]
            for lh, v in samples_of(poses, cov, mine, a, b, sigma_floor_mm, cov_scale, min_length_mm, debias):
                if gate and gate > 0 and len(kept) >= min_count:
                    ls, vs = np.array(kept).T
                    mean, s0 = np.average(ls, weights=1.0 / vs), np.sum(1.0 / vs)
                    r2, threshold = (lh - mean) ** 2, gate * (v + 1.0 / s0)
                    table['margins'].append(abs(r2 - threshold) / threshold)
                    if r2 > threshold:
                        table['rejected'][t, e] += 1
                        continue
                kept.append((lh, v))
    return table


def stats(table):
    """-> float64 [T, E, 4] = (S0, S1, count, rejected), the kernel's table."""
    out = np.zeros((table['T'], table['E'], 4))
    for (t, e), kept in table['samples'].items():
        if kept:
            ls, vs = np.array(kept).T
            out[t, e, :3] = np.sum(1.0 / vs), np.sum(ls / vs), len(kept)
        out[t, e, 3] = table['rejected'][t, e]
    return out


def read_out(table, edge_mirror, fallback=None, min_count=8, symmetric=True):
    """-> (lengths [T, E], sigma [T, E], known uint8 [T, E])."""
    T, E = table['T'], table['E']
    lengths, sigma, known = np.full((T, E), np.nan), np.full((T, E), np.nan), np.zeros((T, E), np.uint8)
    for t in range(T):
        for e in range(E):
            pool = list(table['samples'][t, e])
            m = int(edge_mirror[e]) if symmetric else -1
            if 0 <= m < E and m != e:
                pool += table['samples'][t, m]
            if len(pool) >= min_count and len(pool) > 0:
                ls, vs = np.array(pool).T
                lengths[t, e], sigma[t, e], known[t, e] = np.average(ls, weights=1.0 / vs), np.sqrt(1.0 / np.sum(1.0 / vs)), 1
            elif fallback is not None:
                lengths[t, e] = fallback[e]
    return lengths, sigma, known


def run(case):
    """Every call of a case on a fresh table -> (table, [stats after each call], (lengths, sigma, known) after the last)."""
    table, after = new_table(case['T'], len(case['edges'])), []
    for call in case['calls']:
        update(table, call['poses'], call['cov'], call['rows'], call['starts'], call['ids'], case['edges'], **case['params'])
        after.append(stats(table))
    p = case['params']
    return table, after, read_out(table, case['mirror'], case['fallback'], p['min_count'], p['symmetric'])


def pooled_counts(table, edge_mirror, symmetric):
    out = np.zeros((table['T'], table['E']), np.int64)
    for (t, e), kept in table['samples'].items():
        m = int(edge_mirror[e]) if symmetric else -1
        out[t, e] = len(kept) + (len(table['samples'][t, m]) if 0 <= m < table['E'] and m != e else 0)
    return out


def compare(got_stats, got_out, case, what=''):
    """The issue's bounds for a kernel (host-compiled or launched) against the restatement: count, rejected and known exact;
    S0, S1, lengths and sigma within 1e-9 relative (fp64 rounding over at most 2e4 terms).  Asserts first that the case decides
    nothing on a knife's edge: every gate decision is at least 1e-6 relative from its threshold, and no pooled count is
    min_count - 1 or min_count, where one sample more or less would change `known`.  -> the worst relative deviation."""
    table, after, (lengths, sigma, known) = run(case)
    assert all(m >= 1e-6 for m in table['margins']), (what, min(table['margins']))
    p = case['params']
    counts = pooled_counts(table, case['mirror'], p['symmetric'])
    assert not np.isin(counts, (p['min_count'] - 1, p['min_count'])).any(), (what, 'a pooled count at min_count')
    want = after[-1]
    got_stats = np.asarray(got_stats, np.float64)
    assert np.array_equal(got_stats[..., 2:], want[..., 2:]), (what, 'count / rejected')
    worst = 0.0
    for k in (0, 1):
        dev = np.abs(got_stats[..., k] - want[..., k]) / np.maximum(np.abs(want[..., k]), 1e-300)
        dev = np.where(want[..., k] == got_stats[..., k], 0.0, dev)
        worst = max(worst, float(dev.max()))
    g_len, g_sig, g_known = (np.asarray(x) for x in got_out)
    assert np.array_equal(g_known, known), (what, 'known')
    for g, w in ((g_len, lengths), (g_sig, sigma)):
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, 'NaN pattern')
        f = ~np.isnan(w)
        if f.any():
            worst = max(worst, float((np.abs(g[f] - w[f]) / np.abs(w[f])).max()))
    assert worst <= 1e-9, (what, worst)
    return worst


# ---- cases ---------------------------------------------------------------------------------------------------------------------

def h36m():
    from metro_pose3d_amd.joints import skeleton
    sk = skeleton('h36m')
    return sk, np.asarray(sk.edges, np.int32).reshape(-1, 2), np.asarray(sk.edge_mirror(), np.int32)


def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def psd(rng, shape, scale):
    a = rng.normal(size=shape + (3, 3)) * scale
    return a @ np.swapaxes(a, -1, -2) + (0.25 * scale ** 2) * np.eye(3)


def case_of(calls, edges, mirror, T, fallback=None, **params):
    return dict(calls=calls, edges=np.asarray(edges, np.int32).reshape(-1, 2), mirror=np.asarray(mirror, np.int32), T=T,
                fallback=None if fallback is None else np.asarray(fallback, np.float64), params=dict(DEFAULTS, **params))


def call_of(poses, cov, rows, starts, ids):
    return dict(poses=None if poses is None else np.asarray(poses, np.float32),
                cov=None if cov is None else np.asarray(cov, np.float32).reshape(len(cov), -1, 9),
                rows=np.asarray(rows, np.int32), starts=np.asarray(starts, np.int32), ids=np.asarray(ids, np.int32))


def stream_case(seed, T, E, J, rows_per_slot, steps_per_call=None, nan_joint=None, with_cov=True, **params):
    """Slots 0 .. T-1 each follow one rigid random skeleton of J joints through rows_per_slot[t % len] exposures: a rigid motion per
    row, joint noise of a few mm with a matching covariance, a few joints NaN, a few outliers 200 mm off, a few covariances NaN or
    with a negative variance, and the indices -1 and n among the rows.  steps_per_call: the exposures are cut into calls of that
    many steps (None: one call)."""
    rng = np.random.default_rng([seed, T, E, J])
    edges = np.stack([rng.integers(0, J, E), rng.integers(0, J, E)], 1) if J > 1 else np.zeros((E, 2), np.int64)
    if J > 1:
        same = edges[:, 0] == edges[:, 1]
        edges[same, 1] = (edges[same, 0] + 1) % J
        edges[E // 2] = edges[E // 2, 0]                      # one zero-length edge
    mirror = np.arange(E) ^ 1
    mirror[mirror >= E] = -1
    mirror[::5] = -1                                          # some without a partner (their partners still point at them)
    if E > 3:
        mirror[3] = 3
    counts = [rows_per_slot[t % len(rows_per_slot)] for t in range(T)]
    base = rng.normal(size=(T, J, 3)) * 250.0
    n_steps = max(counts) if counts else 0
    poses, cov, slot_of, step_of = [], [], [], []
    for s in range(n_steps):
        for t in range(T):
            if s >= counts[t]:
                continue
            sigma = rng.uniform(2.0, 9.0)
            c = psd(rng, (J,), sigma)
            noise = np.einsum('jab,jb->ja', np.linalg.cholesky(c), rng.normal(size=(J, 3)))
            p = base[t] @ rotation(rng).T + rng.normal(size=3) * 2000.0 + noise
            if rng.random() < 0.1:
                p[rng.integers(J)] += 200.0
            if rng.random() < 0.15 or (t, s) == (0, 1):       # slot 0 has one row of each kind for certain
                p[rng.integers(J)] = np.nan
            if rng.random() < 0.05 or (t, s) == (0, 2):
                c[rng.integers(J), 0, 2] = np.nan
            if rng.random() < 0.05 or (t, s) == (0, 3):
                c[rng.integers(J), 1, 1] = -4.0
            if nan_joint is not None:
                p[list(nan_joint)] = np.nan
            poses.append(p), cov.append(c), slot_of.append(t), step_of.append(s)
    n = len(poses)
    poses = np.asarray(poses, np.float32).reshape(n, J, 3)
    cov = np.asarray(cov, np.float32).reshape(n, J, 9)
    slot_of, step_of = np.asarray(slot_of, np.int64), np.asarray(step_of, np.int64)
    ids = np.arange(T) + 100
    cuts = [(0, n_steps)] if steps_per_call is None else [(a, min(a + steps_per_call, n_steps)) for a in range(0, n_steps, steps_per_call)]
    calls = []
    for a, b in cuts or [(0, 0)]:
        sel = np.flatnonzero((step_of >= a) & (step_of < b))
        local = {int(r): k for k, r in enumerate(sel)}
        # time order: the rows were appended step by step
        rows = [np.array([local[int(r)] for r in sel[slot_of[sel] == t]], np.int64) for t in range(T)]
        if len(sel):
            rows[0] = np.concatenate([[-1], rows[0], [len(sel)]])            # two indices outside [0, n)
        starts = np.concatenate([[0], np.cumsum([len(g) for g in rows])])
        calls.append(call_of(poses[sel], cov[sel] if with_cov else None, np.concatenate(rows) if rows else [], starts, ids))
    return case_of(calls, edges, mirror, T, fallback=rng.uniform(100, 500, E), **params)


def bias_scene(seed, rows=20000):
    """A 250 mm bone along (0.6, 0, 0.8); joint noise N(0, s^2 diag(8, 8, 30)^2) and N(0, s^2 diag(10, 10, 35)^2) mm, s ~ U(0.5, 3)
    per row; the gate off.  float64 arrays: the known-answer tests feed the restatement directly."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.5, 3.0, rows)
    sa, sb = np.array([8.0, 8.0, 30.0]), np.array([10.0, 10.0, 35.0])
    a = rng.normal(size=(rows, 3)) * 1000.0
    poses = np.stack([a + rng.normal(size=(rows, 3)) * s[:, None] * sa,
                      a + 250.0 * np.array([0.6, 0.0, 0.8]) + rng.normal(size=(rows, 3)) * s[:, None] * sb], 1)
    cov = np.zeros((rows, 2, 3, 3))
    cov[:, 0, [0, 1, 2], [0, 1, 2]] = (s[:, None] * sa) ** 2
    cov[:, 1, [0, 1, 2], [0, 1, 2]] = (s[:, None] * sb) ** 2
    return poses, cov


def bias_case(seed, rows=20000, debias=True):
    poses, cov = bias_scene(seed, rows)
    return case_of([call_of(poses, cov, np.arange(rows), [0, rows], [7])], [[0, 1]], [-1], 1, gate=0.0, debias=debias)


def outlier_case(position):
    """One track of h36m skeletons at sigma = 10 mm per axis and joint pair (C_a + C_b = 100 I): 10 good rows and one in which a leaf joint is
    150 mm off along its bone, inserted at `position`."""
    sk, edges, mirror = h36m()
    rng = np.random.default_rng(5)
    base = rng.normal(size=(sk.n_out, 3)) * 250.0
    good = np.stack([base @ rotation(rng).T + rng.normal(size=3) * 1000.0 + rng.normal(size=(sk.n_out, 3)) * 2.0 for _ in range(11)])
    leaf = [j for j in range(sk.n_out) if (edges == j).sum() == 1][0]           # a joint of one bone only
    bad_edge = int(np.flatnonzero((edges == leaf).any(1))[0])
    other = int(edges[bad_edge][edges[bad_edge] != leaf][0])
    u = (good[position, leaf] - good[position, other]) / np.linalg.norm(good[position, leaf] - good[position, other])
    good[position, leaf] += 150.0 * u
    cov = np.tile(50.0 * np.eye(3), (11, sk.n_out, 1, 1))
    return case_of([call_of(good, cov, np.arange(11), [0, 11], [3])], edges, mirror, 1, symmetric=False), bad_edge


def arm_case(symmetric):
    """h36m, two tracks, 12 exposures; the left arm (lsho, lelb, lwri) NaN throughout."""
    sk, edges, mirror = h36m()
    left = [sk.names.index(n) for n in ('lelb', 'lwri')]
    c = stream_case(11, 2, len(edges), sk.n_out, [12], nan_joint=left, symmetric=symmetric)
    c['edges'], c['mirror'] = edges, mirror
    return c, left


CUTS = (None, 1, 3, 8)
SHAPES = {'T1-E1-J1': (1, 1, 1), 'T2-E16-J17': (2, 16, 17), 'T65-E63-J64': (65, 63, 64), 'T128-E64-J64': (128, 64, 64)}


def shape_case(name):
    T, E, J = SHAPES[name]
    return stream_case(3, T, E, J, [65, 0, 1, 2])


def cut_case(steps_per_call):
    return stream_case(17, 3, 16, 17, [20, 3, 0], steps_per_call)


def forget_case(change):
    """Two calls of 14 exposures; slot 1's id changes between them (`change`) or stays."""
    c = stream_case(23, 2, 16, 17, [28], 14)
    if change:
        c['calls'][1]['ids'] = c['calls'][1]['ids'] + np.array([0, 50], np.int32)
    return c


def isotropic_case():
    return stream_case(29, 3, 16, 17, [40, 3, 30], with_cov=False, sigma_floor_mm=8.0)     # the floor is the whole noise model here
