"""fp64 NumPy restatement of the choice among heat-map modes by bone lengths (metro_plan_bind_skeleton_modes,
include/metro_hip.h), written unlike the kernel, in two forms:
  (a) `enumerate_component`: every assignment of a component listed, its log-probability summed term by term; marginals,
      max-marginals, MAP and both logs read off the list.  Used where the product of the mode counts is at most ENUM_MAX.
  (b) `eliminate_component`: dense variable elimination on [K_parent, K_child] tables with np.logaddexp.reduce / np.max, the
      tree rooted at the component's HIGHEST-numbered joint (the kernel roots at the lowest), messages up, then down.
The two must agree within 1e-12 wherever both apply (`infer(..., form='both')` asserts it).  No schedule, no re-rooting, no
back-pointers: the MAP is the arg-max of the max-marginals, which is the MAP wherever it is unique -- `gap` says by how much.
Also what the tests share: the case generator, the comparison with its bounds, and the forearm scene."""
import itertools

import numpy as np

STATS = 11                      # mass, peak, coords01 (x, y, z), cov01 (xx, yy, zz, xy, xz, yz)
COV6 = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
ENUM_MAX = 20000
MIN_GAP = 1e-6                  # a compared joint's best and second-best max-marginal differ by at least this
PROB_TOL, LOG_TOL = 1e-9, 1e-9  # the bounds the kernel is held to, before its one rounding to fp32
DEFAULTS = dict(sigma_mm=20.0, sigma_rel=0.0, cov_scale=1.0, min_length_mm=1.0)


def cov3(c6):
    m = np.empty((3, 3))
    for v, (a, b) in zip(c6, COV6):
        m[a, b] = m[b, a] = v
    return m


def potentials(voxel, stats, lengths, edges, scale_mm, sigma_mm, sigma_rel, cov_scale, min_length_mm):
    """One crop row -> present [J, K], ln w [J, K] (-inf where absent), w [J, K], known [E], ln psi [E, K, K] (0 where unused)."""
    voxel, stats = np.asarray(voxel), np.asarray(stats, np.float64)
    nj, k = voxel.shape
    a = np.asarray(scale_mm, np.float64)
    present = (voxel >= 0) & np.isfinite(stats[..., 0]) & (stats[..., 0] > 0) & np.isfinite(stats[..., 2:]).all(-1)
    alive = present.any(-1)
    w = np.zeros((nj, k))
    for j in np.flatnonzero(alive):
        w[j, present[j]] = stats[j, present[j], 0] / stats[j, present[j], 0].sum()
    with np.errstate(divide='ignore'):
        lnw = np.where(present, np.log(np.where(present, w, 1.0)), -np.inf)
    known = np.zeros(len(edges), bool)
    lnpsi = np.zeros((len(edges), k, k))
    for e, (p, q) in enumerate(edges):
        big = lengths[e]
        known[e] = np.isfinite(big) and big > 0 and alive[p] and alive[q]
        if not known[e]:
            continue
        v0 = sigma_mm ** 2 + (sigma_rel * big) ** 2
        for ka, kb in itertools.product(np.flatnonzero(present[p]), np.flatnonzero(present[q])):
            d = a * stats[q, kb, 2:5] - a * stats[p, ka, 2:5]
            ell = np.linalg.norm(d)
            cov = (cov3(stats[p, ka, 5:]) + cov3(stats[q, kb, 5:])) * np.outer(a, a)
            s = np.trace(cov) / 3 if (ell < min_length_mm or ell == 0) else (d / ell) @ cov @ (d / ell)
            v = v0 + cov_scale * max(0.0, s)
            lnpsi[e, ka, kb] = -(ell - big) ** 2 / (2 * v) - 0.5 * np.log(v / v0)
    return present, lnw, w, known, lnpsi


def components(nj, edges, known, alive):
    """The sorted joint lists of the maximal sets of alive joints joined by known edges."""
    label = list(range(nj))
    for e, (p, q) in enumerate(edges):
        if known[e]:
            lp, lq = label[p], label[q]
            label = [lp if v == lq else v for v in label]
    groups = {}
    for j in range(nj):
        if alive[j]:
            groups.setdefault(label[j], []).append(j)
    return sorted(groups.values())


def enumerate_component(joints, comp_edges, present, lnw, lnpsi):
    """(a).  comp_edges: (e, p, q) of the component's known edges.  -> (log marginals [n, K], max-marginals [n, K], log Z)"""
    options = [np.flatnonzero(present[j]) for j in joints]
    at = {j: i for i, j in enumerate(joints)}
    grids = np.meshgrid(*options, indexing='ij')
    assign = np.stack([g.reshape(-1) for g in grids], axis=1)                     # [A, n]
    logp = np.zeros(len(assign))
    for i, j in enumerate(joints):
        logp = logp + lnw[j, assign[:, i]]
    for e, p, q in comp_edges:
        logp = logp + lnpsi[e, assign[:, at[p]], assign[:, at[q]]]
    k = present.shape[1]
    log_z = np.logaddexp.reduce(logp)
    marg, maxm = np.full((len(joints), k), -np.inf), np.full((len(joints), k), -np.inf)
    for i in range(len(joints)):
        for m in options[i]:
            rows = logp[assign[:, i] == m]
            marg[i, m], maxm[i, m] = np.logaddexp.reduce(rows) - log_z, rows.max() - log_z
    return marg, maxm, log_z


def eliminate_component(joints, comp_edges, present, lnw, lnpsi):
    """(b).  Same outputs as (a)."""
    root = max(joints)
    table = {}                                                                     # (parent, child) -> [K_parent, K_child]
    nbrs = {j: [] for j in joints}
    for e, p, q in comp_edges:
        nbrs[p].append(q)
        nbrs[q].append(p)
        table[(p, q)], table[(q, p)] = lnpsi[e], lnpsi[e].T
    order, parent = [root], {root: None}
    for j in order:                                                                # breadth first from the root
        for c in nbrs[j]:
            if c not in parent:
                parent[c] = j
                order.append(c)
    out = []
    for reduce_ in (np.logaddexp.reduce, np.max):
        up, below = {}, {j: lnw[j].copy() for j in joints}                         # below: the unary and all messages from the children
        for c in reversed(order[1:]):
            with np.errstate(invalid='ignore'):
                up[c] = reduce_(table[(parent[c], c)] + below[c][None, :], axis=1)
            below[parent[c]] = below[parent[c]] + up[c]
        belief = {root: below[root]}
        for c in order[1:]:
            p = parent[c]
            with np.errstate(invalid='ignore'):
                rest = np.where(present[p], belief[p] - up[c], -np.inf)            # the parent's belief without this child's message
                belief[c] = below[c] + reduce_(table[(p, c)] + rest[:, None], axis=0)
        out.append(belief)
    log_z = np.logaddexp.reduce(out[0][root])
    marg = np.stack([out[0][j] for j in joints]) - log_z
    maxm = np.stack([out[1][j] for j in joints]) - log_z
    return marg, maxm, log_z


def infer_row(voxel, stats, lengths, edges, scale_mm, form='auto', **options):
    """One crop row -> dict(prob [J, K], choice [J], log_evidence [J], log_map [J], gap [J], maxm [J, K]).  form: 'auto' ((a)
    where it applies, else (b)), 'enumerate', 'eliminate', or 'both' ((a) and (b) where (a) applies, asserted equal within
    1e-12, else (b))."""
    opt = dict(DEFAULTS, **options)
    present, lnw, w, known, lnpsi = potentials(voxel, stats, lengths, edges, scale_mm, **opt)
    nj, k = present.shape
    alive = present.any(-1)
    res = dict(prob=np.full((nj, k), np.nan), choice=np.full(nj, -1, np.int32), log_evidence=np.full(nj, np.nan),
               log_map=np.full(nj, np.nan), gap=np.full(nj, np.inf), maxm=np.full((nj, k), np.nan))
    for joints in components(nj, edges, known, alive):
        inside = set(joints)
        comp_edges = [(e, p, q) for e, (p, q) in enumerate(edges) if known[e] and p in inside]
        if not comp_edges:                                                         # one joint: its unaries, an evidence of exactly 1
            j = joints[0]
            marg, maxm, log_z = lnw[j][None], lnw[j][None], 0.0
            prob = w[j][None]
        else:
            small = np.prod([float(present[j].sum()) for j in joints]) <= ENUM_MAX
            if form == 'enumerate' or (form in ('auto', 'both') and small):
                marg, maxm, log_z = enumerate_component(joints, comp_edges, present, lnw, lnpsi)
                if form == 'both':
                    other = eliminate_component(joints, comp_edges, present, lnw, lnpsi)
                    for x, y in zip((marg, maxm), other[:2]):
                        fin = np.isfinite(x)
                        assert np.array_equal(fin, np.isfinite(y)) and np.abs(x[fin] - y[fin]).max() <= 1e-12, np.abs(x[fin] - y[fin]).max()
                    assert abs(log_z - other[2]) <= 1e-12
            else:
                marg, maxm, log_z = eliminate_component(joints, comp_edges, present, lnw, lnpsi)
            prob = np.exp(marg)
        for i, j in enumerate(joints):
            res['prob'][j] = np.where(present[j], prob[i], 0.0)
            res['maxm'][j] = maxm[i]
            ranked = np.sort(maxm[i][present[j]])[::-1]
            res['choice'][j] = int(np.argmax(maxm[i]))
            res['gap'][j] = ranked[0] - ranked[1] if len(ranked) > 1 else np.inf
            res['log_evidence'][j] = log_z
            res['log_map'][j] = maxm[i].max()
    return res


def infer(voxel, stats, lengths, edges, scale_mm, form='auto', **options):
    """Rows [n, ...] -> the same dict with a leading row axis."""
    rows = [infer_row(voxel[i], stats[i], lengths[i], edges, scale_mm, form, **options) for i in range(len(voxel))]
    return {key: np.stack([r[key] for r in rows]) for key in rows[0]}


def assignment_log_prob(choice, voxel, stats, lengths, edges, scale_mm, **options):
    """ln of the UNNORMALISED probability prod w prod psi of one row's assignment, per joint the value of its component; NaN for
    a dead joint (for the tie case: every optimum shares it)."""
    opt = dict(DEFAULTS, **options)
    present, lnw, _, known, lnpsi = potentials(voxel, stats, lengths, edges, scale_mm, **opt)
    nj = len(choice)
    out = np.full(nj, np.nan)
    for joints in components(nj, edges, known, present.any(-1)):
        total = sum(lnw[j, choice[j]] for j in joints)
        total += sum(lnpsi[e, choice[p], choice[q]] for e, (p, q) in enumerate(edges) if known[e] and p in set(joints))
        out[joints] = total
    return out


def select_coords01(coords01, stats, choice, permutation):
    """coords01 [n, Jhead, 3] fp32 with head joint permutation[r] replaced by the chosen mode's coords01 (fp32, as stored)."""
    sel = np.array(coords01, np.float32, copy=True)
    for i, r in itertools.product(range(len(sel)), range(len(permutation))):
        if choice[i, r] >= 0:
            sel[i, permutation[r]] = np.asarray(stats, np.float32)[i, r, choice[i, r], 2:5]
    return sel


# ---- cases ---------------------------------------------------------------------------------------------------------------------

SCALE = (2053.9, 2053.9, 2200.0)             # heatmap_to_metric's linear part of an h36m stride-16 model, mm per coords01 unit


def chain(nj):
    return [(j, j + 1) for j in range(nj - 1)]


def star(nj):
    return [(0, j) for j in range(1, nj)]


def random_tree(rng, nj, n_edges=None):
    """A random forest on nj joints with n_edges edges (default nj - 1: a tree), in random order and orientation."""
    order = rng.permutation(nj)
    edges = [(int(order[rng.integers(0, i)]), int(order[i])) for i in range(1, nj)]
    edges = [e if rng.random() < 0.5 else e[::-1] for e in edges]
    rng.shuffle(edges)
    return edges[:nj - 1 if n_edges is None else n_edges]


def make_case(seed, rows, nj, k, edges, missing=0.15, dead=0.05, unknown=0.1, n_head=None):
    """Hand-filled mode buffers: voxel int32 [rows, nj, k], stats fp32 [rows, nj, k, 11], lengths fp64 [rows, E], coords01 fp32
    [rows, n_head, 3] and a permutation.  Every joint's first mode lies on a random pose whose bone lengths (a little off) are the
    row's lengths; the other modes are elsewhere; masses are random, so the heaviest mode is often a wrong one."""
    rng = np.random.default_rng(seed)
    ne = len(edges)
    voxel = rng.integers(0, 2048, (rows, nj, k)).astype(np.int32)
    stats = np.zeros((rows, nj, k, STATS), np.float32)
    stats[..., 0] = rng.uniform(0.05, 1.0, (rows, nj, k)) / k
    stats[..., 1] = stats[..., 0] * 0.3
    stats[..., 2:5] = rng.uniform(0.05, 0.95, (rows, nj, k, 3))
    sd = rng.uniform(0.005, 0.04, (rows, nj, k, 3))
    rho = rng.uniform(-0.5, 0.5, (rows, nj, k, 3))
    stats[..., 5:8] = sd ** 2
    for i, (a, b) in enumerate(COV6[3:]):
        stats[..., 8 + i] = rho[..., i] * sd[..., a] * sd[..., b]
    pose = stats[..., 0, 2:5].astype(np.float64) * np.asarray(SCALE)
    lengths = np.empty((rows, ne))
    for e, (p, q) in enumerate(edges):
        lengths[:, e] = np.linalg.norm(pose[:, q] - pose[:, p], axis=-1) + rng.normal(0, 15.0, rows)
    lengths = np.abs(lengths) + 1.0
    swap = rng.integers(0, k, (rows, nj))                                          # the true mode is not always mode 0
    for i, j in itertools.product(range(rows), range(nj)):
        stats[i, j, [0, swap[i, j]]] = stats[i, j, [swap[i, j], 0]]
    gone = rng.random((rows, nj, k)) < missing
    gone[rng.random((rows, nj)) < dead] = True
    voxel[gone] = -1
    stats[gone] = np.nan
    stats[gone, 0] = 0.0
    lengths[rng.random((rows, ne)) < unknown] = np.nan
    n_head = nj if n_head is None else n_head
    perm = [int(v) for v in rng.permutation(n_head)[:nj]]
    coords01 = rng.uniform(0, 1, (rows, n_head, 3)).astype(np.float32)
    return dict(voxel=voxel, stats=stats, lengths=lengths, edges=[tuple(e) for e in edges], coords01=coords01, perm=perm, k=k, nj=nj,
                n_head=n_head, rows=rows)


def compare(got, case, ref, what='', wide=True, skip_close=False):
    """got: dict(prob, choice, info, sel) from the code under test.  choice exact; prob within PROB_TOL; both logs within
    LOG_TOL * max(1, |value|) -- for `wide` outputs (fp64, before the one rounding to fp32); for fp32 outputs the same bounds
    hold against the restatement rounded to fp32 once, plus that rounding's own half ulp; coords01_sel exact.  Every compared
    joint must first have a max-marginal gap of at least MIN_GAP in the restatement (skip_close: such joints are left out of the
    choice comparison only, and there may be at most one in a thousand)."""
    close = ref['gap'] < MIN_GAP
    if skip_close:
        assert close.mean() <= 1e-3, (what, int(close.sum()), close.size)
    else:
        assert not close.any(), (what, 'the restatement has a joint whose best two max-marginals are closer than MIN_GAP', ref['gap'].min())
    choice = np.asarray(got['choice'])
    assert np.array_equal(choice[~close], ref['choice'][~close]), (what, 'choice', int((choice != ref['choice'])[~close].sum()))
    prob, info = np.asarray(got['prob'], np.float64), np.asarray(got['info'], np.float64)
    logs = np.stack([ref['log_evidence'], ref['log_map']], -1)
    assert np.array_equal(np.isnan(prob), np.isnan(ref['prob'])) and np.array_equal(np.isnan(info), np.isnan(logs)), (what, 'NaN pattern')
    half_ulp = 0.0 if wide else 2.0 ** -24
    ok = ~np.isnan(ref['prob'])
    dp = np.abs(prob[ok] - ref['prob'][ok]).max() if ok.any() else 0.0
    assert dp <= PROB_TOL + half_ulp, (what, 'prob', dp)
    assert (prob[ok & (ref['prob'] == 0)] == 0).all(), (what, 'absent modes')
    ok = ~np.isnan(logs)
    bound = LOG_TOL * np.maximum(1.0, np.abs(logs[ok])) + half_ulp * np.abs(logs[ok])
    dl = np.abs(info[ok] - logs[ok])
    assert (dl <= bound).all(), (what, 'logs', dl.max())
    edgeless = ok[..., 0] & (ref['log_evidence'] == 0.0)
    assert (info[..., 0][edgeless] == 0.0).all(), (what, 'log_evidence of a component without a known edge must be exactly 0.0')
    assert (info[..., 0][ok[..., 0]] <= 0).all(), (what, 'log_evidence <= 0')
    if got.get('sel') is not None and not close.any():
        want = select_coords01(case['coords01'], case['stats'], ref['choice'], case['perm'])
        assert np.array_equal(np.asarray(got['sel']), want), (what, 'coords01_sel')
    print(f'skeleton_modes {what}: prob {dp:.2e}, logs {dl.max() if dl.size else 0.0:.2e}, least gap {ref["gap"].min():.2e}, '
          f'{int(close.sum())} close of {close.size}')
    return dp, (dl.max() if dl.size else 0.0)


# ---- the forearm scene -----------------------------------------------------------------------------------------------

SCENE = dict(side=16, depth=8, scale=SCALE, shoulder=(900.0, 700.0, 1100.0), elbow_off=(0.0, 280.0, 0.0), wrist_off=(200.0, 150.0, 0.0),
             wrong_dx=-685.0, mass=(0.45, 0.55), bones=(280.0, 250.0), sigma_mm=20.0, k=2, radius=1)


def scene_logits(sd_mm):
    """Three joints (shoulder, elbow, wrist) as Gaussian blobs of sd `sd_mm` on the grid of the soft-argmax -> logits [1, S, S, D*3]
    and the true wrist, the wrong wrist (mm)."""
    from tests.heat_modes_ref import lin01
    s, d, a = SCENE['side'], SCENE['depth'], np.asarray(SCENE['scale'])
    gs, gd = lin01(s), lin01(d)
    pts = np.stack(np.broadcast_arrays(gs[None, :, None] * a[0], gs[:, None, None] * a[1], gd[None, None, :] * a[2]), -1)   # [y, x, d, 3]
    blob = lambda c: np.exp(-0.5 * (((pts - np.asarray(c)) / sd_mm) ** 2).sum(-1))
    shoulder = np.asarray(SCENE['shoulder'])
    elbow = shoulder + SCENE['elbow_off']
    wrist = elbow + SCENE['wrist_off']
    wrong = wrist + (SCENE['wrong_dx'], 0.0, 0.0)
    norm = lambda b: b / b.sum()
    vols = [norm(blob(shoulder)), norm(blob(elbow)), SCENE['mass'][0] * norm(blob(wrist)) + SCENE['mass'][1] * norm(blob(wrong))]
    with np.errstate(divide='ignore'):
        lg = np.log(np.stack(vols, -1))                                           # [S, S, D, 3]
    return lg.reshape(1, s, s, d * 3), wrist, wrong
