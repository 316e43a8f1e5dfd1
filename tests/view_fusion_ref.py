"""fp64 NumPy restatement of the view fusion (metro_plan_bind_view_fusion, include/metro_hip.h), written unlike the kernel: the
grid is a dense meshgrid, K is np.linalg.inv of the stored inverse, the bilinear value is the sum of four weighted cells, the
rows of a person are a Python list, and the moments are matrix products.  TEST INFRASTRUCTURE: the product never imports it.
Also what the tests share: the synthetic rigs and heat-maps, the case builder, the margins that keep every compared case away
from a decision the tolerance could flip, and the bounds of the issue."""
from typing import NamedTuple

import numpy as np

from metro_pose3d_amd import _lib

PLACEMENT = np.dtype(_lib.MetroPlacement)
DEFAULTS = dict(grid=16, n_views=1, extent_mm=1200.0, floor=1e-6, near_mm=100.0)

# the bounds the tests hold (both sides compute in fp64 on the same fp32 inputs and round once to fp32)
POINT_MM = 1e-3                 # the project's parity bar for fp64 paths (triangulation_ref.PARITY_MM)
BLOCK_BOUND = 1e-6              # each covariance block within this of its largest entry
STAT_ULPS, STAT_ABS = 4, 1e-6   # peak and agreement: 4 fp32 ulps or 1e-6
BORDER_MARGIN_CELLS, NEAR_MARGIN_MM, LEAD_MARGIN = 1e-6, 1e-3, 1e-9


class Head(NamedTuple):
    """What the fusion needs of a model's head: the heat-map side and heatmap_to_image's two constants."""
    side: int
    lrc: float
    half_off: float


def head_of(proc_side: int, stride: int, centered: bool = True) -> Head:
    last = proc_side - 1
    return Head(proc_side // stride, float(last - last % stride - 1), float(stride // 2 if centered else 0))


def cspec(head_side: int, n_out: int, stride: int = 16, centered: bool = True):
    """A MetroSpec with the fields the fusion launch reads (proc_side, stride, centered_stride, n_joints_out) and the Head of it."""
    cs = _lib.MetroSpec()
    cs.stride, cs.proc_side, cs.centered_stride, cs.n_joints_out = stride, head_side * stride, int(centered), n_out
    cs.n_joints_head, cs.depth, cs.box_size_mm = n_out, 8, 2200.0
    for r in range(n_out):
        cs.permutation[r] = r
    return cs, head_of(cs.proc_side, stride, centered)


# ---- the restatement -------------------------------------------------------------------------------------------------------------

def _sample(head: Head, rec, heat, pts, near, floor):
    """One row at the world points pts [N, 3] -> (ln max(p, floor) [N], border margin in cells, near margin in mm)."""
    s = head.side
    k = np.linalg.inv(np.asarray(rec['inv_intrinsics'], np.float64).reshape(3, 3))
    rot = np.asarray(rec['rot_to_world'], np.float64).reshape(3, 3)
    cam = (pts - np.asarray(rec['cam_loc'], np.float64)) @ rot                      # rot^T (X - o), row by row
    with np.errstate(invalid='ignore', divide='ignore'):
        front = cam[:, 2] > near
        h = np.stack([cam[:, 0] / cam[:, 2], cam[:, 1] / cam[:, 2], np.ones(len(cam))], axis=1) @ k.T
        f = (h[:, :2] - head.half_off) / head.lrc * (s - 1)
        inside = front & (f[:, 0] >= 0) & (f[:, 0] <= s - 1) & (f[:, 1] >= 0) & (f[:, 1] <= s - 1)
    out = np.full(len(pts), np.log(floor))
    fi = f[inside]
    x0 = np.minimum(np.floor(fi[:, 0]).astype(np.int64), s - 2)
    y0 = np.minimum(np.floor(fi[:, 1]).astype(np.int64), s - 2)
    tx, ty = fi[:, 0] - x0, fi[:, 1] - y0
    m = np.asarray(heat, np.float64)
    p = (1 - tx) * (1 - ty) * m[y0, x0] + tx * (1 - ty) * m[y0, x0 + 1] + (1 - tx) * ty * m[y0 + 1, x0] + tx * ty * m[y0 + 1, x0 + 1]
    p = np.minimum(p, m.max())                          # a bilinear value is never above the map's largest cell
    out[inside] = np.log(np.maximum(p, floor))
    ff = f[front & np.isfinite(f).all(axis=1)]
    border = np.abs(np.concatenate([ff, ff - (s - 1)], axis=1)).min(initial=np.inf)
    return out, float(border), float(np.abs(cam[:, 2] - near).min(initial=np.inf))


def fuse(case):
    """-> dict(points [P, Jout, 3], cov [P, Jout, 3, 3], peak, agreement [P, Jout] float64; n_rows, edge [P, Jout] int32;
    margins: dict(border, near, lead), the least of each over the case)."""
    head, par = case['head'], dict(DEFAULTS, **case.get('params', {}))
    g_n, views, extent, floor, near = par['grid'], par['n_views'], par['extent_mm'], par['floor'], par['near_mm']
    xy, records, mirror, n = case['xy'], case['records'], list(case['mirror']), case['n']
    rows, starts = [int(v) for v in case['rows']], [int(v) for v in case['starts']]
    n_persons, n_out = len(starts) - 1, len(mirror)
    centres = np.asarray(case['centres'], np.float32).astype(np.float64)
    out = dict(points=np.full((n_persons, n_out, 3), np.nan), cov=np.full((n_persons, n_out, 3, 3), np.nan),
               peak=np.full((n_persons, n_out), np.nan), agreement=np.full((n_persons, n_out), np.nan),
               n_rows=np.zeros((n_persons, n_out), np.int32), edge=np.zeros((n_persons, n_out), np.int32))
    margins = dict(border=np.inf, near=np.inf, lead=np.inf)
    g = -extent / 2 + np.arange(g_n) * (extent / (g_n - 1))
    offsets = np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)          # v = (a G + b) G + c
    for p in range(n_persons):
        group = rows[max(starts[p], 0):min(starts[p + 1], len(rows))]
        for r in range(n_out):
            if not np.isfinite(centres[p, r]).all():
                continue
            pts = centres[p, r] + offsets
            logs, tops = [], []
            for i in group:
                if not 0 <= i < n:
                    continue
                rec = records[i]
                if not all(np.isfinite(np.asarray(rec[name], np.float64)).all() for name in ('inv_intrinsics', 'rot_to_world', 'cam_loc')):
                    continue
                flipped = not np.linalg.det(np.asarray(rec['rot_to_world'], np.float64).reshape(3, 3)) > 0
                src = mirror[r] if flipped else r
                if not 0 <= src < n_out or not np.isfinite(xy[i, src]).all():
                    continue
                l, border, near_margin = _sample(head, rec, xy[i, src], pts, near, floor)
                logs.append(l)
                tops.append(np.log(max(float(xy[i, src].max()), floor)))
                margins['border'], margins['near'] = min(margins['border'], border), min(margins['near'], near_margin)
            if not logs:
                continue
            e = np.sum(logs, axis=0) / views
            best = int(np.argmax(e))                                # the first of equals: the lowest v
            if len(e) > 1:
                margins['lead'] = min(margins['lead'], float(e[best] - np.delete(e, best).max()))
            w = np.exp(e - e[best])
            w = w / w.sum()
            mean = w @ pts
            d = pts - mean
            a, b, c = best // (g_n * g_n), best // g_n % g_n, best % g_n
            out['points'][p, r], out['cov'][p, r] = mean, (w[:, None] * d).T @ d
            out['peak'][p, r], out['agreement'][p, r] = w.max(), e[best] - np.sum(tops) / views
            out['n_rows'][p, r], out['edge'][p, r] = len(logs), int(any(t in (0, g_n - 1) for t in (a, b, c)))
    out['margins'] = margins
    return out


def assert_margins(ref):
    """Every projection at least 1e-6 cells from the map border and 1e-3 mm from near_mm, and the largest E ahead of every other
    point by 1e-9: no decision of the compared case can flip between two fp64 evaluations."""
    m = ref['margins']
    assert m['border'] >= BORDER_MARGIN_CELLS and m['near'] >= NEAR_MARGIN_MM and m['lead'] >= LEAD_MARGIN, m


def check(got, ref):
    """The outputs of the code under test -- (points [P, Jout, 3], cov [P, Jout, 9], stats [P, Jout, 2], info [P, Jout, 2]) -- against
    the restatement's: integers exact, the same NaN pattern, and the bounds above.  -> the worst deviations."""
    points, cov, stats, info = (np.asarray(a) for a in got)
    assert_margins(ref)
    assert info.dtype == np.int32 and np.array_equal(info[..., 0], ref['n_rows']) and np.array_equal(info[..., 1], ref['edge']), \
        (info[..., 0], ref['n_rows'], info[..., 1], ref['edge'])
    none = np.isnan(ref['peak'])
    assert np.array_equal(none, ref['n_rows'] == 0)
    for name, a in (('points', points), ('cov', cov), ('stats', stats)):
        assert a.dtype == np.float32 and np.array_equal(np.isnan(a), np.broadcast_to(none[..., None], a.shape)), name
    worst = dict(points_mm=0.0, block=0.0, peak=0.0, agreement=0.0)
    if none.all():
        return worst
    ok = ~none
    worst['points_mm'] = float(np.abs(points[ok].astype(np.float64) - ref['points'][ok]).max())
    assert worst['points_mm'] <= POINT_MM, worst
    want = ref['cov'][ok].reshape(-1, 9)
    dev = np.abs(cov[ok].astype(np.float64) - want).max(axis=1) / np.abs(want).max(axis=1)
    worst['block'] = float(dev.max())
    assert worst['block'] <= BLOCK_BOUND, worst
    for k, name in enumerate(('peak', 'agreement')):
        w = ref[name][ok]
        bound = np.maximum(STAT_ULPS * np.spacing(np.abs(w).astype(np.float32)).astype(np.float64), STAT_ABS)
        dev = np.abs(stats[..., k][ok].astype(np.float64) - w)
        worst[name] = float(dev.max())
        assert (dev <= bound).all(), (name, worst)
    assert (stats[..., 1][ok] <= 0).all() and (stats[..., 0][ok] > 0).all() and (stats[..., 0][ok] <= 1).all()
    return worst


# ---- synthetic rigs and heat-maps ------------------------------------------------------------------------------------------------

def look_at(position, target=(0.0, 0.0, 0.0)):
    """rot_to_world (camera axes as columns, det +1) of a camera at `position` looking at `target`, world z up."""
    position, target = np.asarray(position, np.float64), np.asarray(target, np.float64)
    z = (target - position) / np.linalg.norm(target - position)
    up = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.99 else np.array([0.0, 1.0, 0.0])
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z], axis=1)


def record(k, rot_to_world, cam_loc):
    rec = np.zeros((), PLACEMENT)
    rec['inv_intrinsics'] = np.linalg.inv(np.asarray(k, np.float64)).astype(np.float32).reshape(-1)
    rec['rot_to_world'] = np.asarray(rot_to_world, np.float64).astype(np.float32).reshape(-1)
    rec['cam_loc'] = np.asarray(cam_loc, np.float64).astype(np.float32)
    return rec


def ring_records(angles_deg, side_px, radius=4500.0, height=0.0, target=(0.0, 0.0, 0.0), span_mm=2200.0):
    """One record per angle: a pinhole camera on a circle of `radius` about `target` whose crop of side_px pixels spans span_mm
    at the target (f = side_px radius / span_mm, the principal point in the middle)."""
    f = side_px * radius / span_mm
    k = np.array([[f, 0, side_px / 2], [0, f, side_px / 2], [0, 0, 1.0]])
    recs = np.zeros(len(angles_deg), PLACEMENT)
    for i, ang in enumerate(np.radians(angles_deg)):
        o = np.asarray(target, np.float64) + np.array([radius * np.cos(ang), radius * np.sin(ang), height])
        recs[i] = record(k, look_at(o, target), o)
    return recs


def cells_of(head: Head, rec, pts):
    """World points [..., 3] -> their heat-map cell coordinates f = m (S - 1) [..., 2] in the row's map (fp64, the stored record)."""
    k = np.linalg.inv(np.asarray(rec['inv_intrinsics'], np.float64).reshape(3, 3))
    cam = (np.asarray(pts, np.float64) - np.asarray(rec['cam_loc'], np.float64)) @ np.asarray(rec['rot_to_world'], np.float64).reshape(3, 3)
    px = cam @ k.T
    return (px[..., :2] / px[..., 2:] - head.half_off) / head.lrc * (head.side - 1)


def blob(head: Head, at, sd=0.8):
    """A Gaussian blob of sd cells at cell coordinates `at` (x, y), summing to 1: float64 [S, S] indexed [y, x]."""
    c = np.arange(head.side, dtype=np.float64)
    m = np.exp(-0.5 * ((c[None, :] - at[0]) ** 2 + (c[:, None] - at[1]) ** 2) / sd ** 2)
    return m / m.sum()


def map_moments(head: Head, m):
    """The soft-argmax of an xy map: (mean01 (x, y), cov01 xx, yy) on the grid linspace(0, 1, S)."""
    g = np.linspace(0.0, 1.0, head.side)
    px, py = m.sum(axis=0), m.sum(axis=1)
    mx, my = px @ g, py @ g
    return np.array([mx, my]), px @ (g - mx) ** 2, py @ (g - my) ** 2


def triangulate_means(head: Head, records, means01, var01, weighted: bool):
    """The point nearest to the rays through the maps' means (metro_triangulate_joints' two solves, for the scene tests):
    uniform, or a second solve with w = 1 / (sigma^2 z^2), sigma^2 = (var_xx + var_yy) / 2 lrc^2 inv_intrinsics[0]^2."""
    ds, os_, s2 = [], [], []
    for rec, m01, v01 in zip(records, means01, var01):
        ki = np.asarray(rec['inv_intrinsics'], np.float64).reshape(3, 3)
        uv = np.asarray(m01) * head.lrc + head.half_off
        d = np.asarray(rec['rot_to_world'], np.float64).reshape(3, 3) @ (ki @ np.array([uv[0], uv[1], 1.0]))
        ds.append(d / np.linalg.norm(d))
        os_.append(np.asarray(rec['cam_loc'], np.float64))
        s2.append(0.5 * (v01[0] + v01[1]) * head.lrc ** 2 * ki[0, 0] ** 2)
    ds, os_, s2 = np.array(ds), np.array(os_), np.array(s2)

    def solve(w):
        proj = np.eye(3)[None] - ds[:, :, None] * ds[:, None, :]
        return np.linalg.solve((w[:, None, None] * proj).sum(axis=0), (w[:, None] * np.einsum('kab,kb->ka', proj, os_)).sum(axis=0))
    x = solve(np.ones(len(ds)))
    if weighted:
        z = np.einsum('ka,ka->k', ds, x[None] - os_)
        x = solve(1.0 / (s2 * z * z))
    return x


SCENE_HEAD = Head(16, 240.0, 8.0)            # the issue's scene: S = 16, side 256, lrc 240, half_off 8
SCENE_TRUTH = np.array([100.0, 50.0, -30.0])


def scene(angles_deg=(0.0, 120.0, 240.0), wrong_weight=0.55, wrong_cells=5.0, params=None):
    """The issue's scene: pinhole cameras on a circle of 4.5 m (f = 256 . 4500 / 2200 px), the true joint at (100, 50, -30) mm,
    each map a blob of sd 0.8 cells at the true projection; camera 0 carries `wrong_weight` of its mass in a second blob
    wrong_cells to the right.  -> (the fusion case of one person and one joint, centred on the covariance-weighted
    triangulation of the means as the product centres it, the uniform triangulation, the covariance-weighted one)."""
    head = SCENE_HEAD
    recs = ring_records(angles_deg, 256.0)
    maps, means, variances = [], [], []
    for i, rec in enumerate(recs):
        at = cells_of(head, rec, SCENE_TRUTH)
        m = blob(head, at)
        if i == 0 and wrong_weight > 0:
            m = (1 - wrong_weight) * m + wrong_weight * blob(head, at + np.array([wrong_cells, 0.0]))
        m = m.astype(np.float32)
        mean, vx, vy = map_moments(head, m.astype(np.float64))
        maps.append(m), means.append(mean), variances.append((vx, vy))
    uniform = triangulate_means(head, recs, means, variances, False)
    weighted = triangulate_means(head, recs, means, variances, True)
    xy = np.stack(maps)[:, None]
    case = dict(head=head, xy=xy, records=recs, rows=list(range(len(recs))), starts=[0, len(recs)], mirror=[0], n=len(recs),
                centres=weighted.astype(np.float32)[None, None], params=dict(DEFAULTS, **(params or {})))
    return case, uniform, weighted


# ---- the cases the kernel's code is held to, on the host (test_view_fusion.py) and on the GPU (test_gpu_view_fusion.py) ----------

def pair_mirror(n_out):
    """An output-order mirror table: joints 0 <-> 1, 2 <-> 3, ...; an odd last joint is its own mirror."""
    m = np.arange(n_out, dtype=np.int32)
    m[:n_out // 2 * 2] ^= 1
    return m


def make_case(head: Head, n_out=3, rows_per_person=(3,), n_views=1, grid=16, extent_mm=1200.0, seed=0, stride=16, spare_rows=1,
              centre_noise_mm=40.0, mirror=None, flip_rows=(), **params):
    """Persons with rows_per_person[p] crop rows each, cameras on a ring about the person at uneven angles, every map a blob
    at the joint's projection plus a weaker second blob elsewhere and a little noise (no two cells equal, no symmetry the
    argmax could tie on); the crop rows are stored in a scrambled order with spare_rows unused ones; the centres are the
    true joints moved by centre_noise_mm.  flip_rows: the rows (counted over all persons) that are flipped views -- rot_to_world
    with its x axis turned round, det -1 -- whose maps are stored under the mirror joints."""
    rng = np.random.default_rng(seed)
    mir = pair_mirror(n_out) if mirror is None else np.asarray(mirror, np.int32)
    n_persons, total = len(rows_per_person), int(sum(rows_per_person))
    n = total + spare_rows
    store = rng.permutation(n)[:total]                         # where each (person, camera) row is stored
    xy = rng.uniform(1e-5, 2e-5, (n, n_out, head.side, head.side))
    records = ring_records(rng.uniform(0, 360, n), head.side * stride)
    truth = rng.uniform(-250, 250, (n_persons, n_out, 3)) + rng.uniform(-300, 300, (n_persons, 1, 3))
    rows, starts, k = [], [0], 0
    for p, cnt in enumerate(rows_per_person):
        angles = (np.arange(cnt) * (360.0 / max(cnt, 1)) + rng.uniform(-15, 15, cnt) + 37.0 * p) % 360
        recs = ring_records(angles, head.side * stride, radius=4500.0 + 100.0 * p, height=300.0 * (p % 3) - 200.0,
                            target=truth[p].mean(axis=0))
        for c in range(cnt):
            i = int(store[k])
            flipped = k in flip_rows
            k += 1
            if flipped:
                recs[c]['rot_to_world'] = (recs[c]['rot_to_world'].reshape(3, 3) * np.array([-1, 1, 1], np.float32)[None, :]).reshape(-1)
            records[i] = recs[c]
            for r in range(n_out):
                at = cells_of(head, recs[c], truth[p, r])
                other = rng.uniform(0, head.side - 1, 2)
                xy[i, mir[r] if flipped else r] += 0.7 * blob(head, at) + 0.3 * blob(head, other)
            rows.append(i)
        starts.append(len(rows))
    xy /= xy.sum(axis=(2, 3), keepdims=True)
    centres = (truth + rng.normal(0, centre_noise_mm, truth.shape)).astype(np.float32)
    return dict(head=head, xy=np.ascontiguousarray(xy, np.float32), records=records, rows=np.asarray(rows, np.int32),
                starts=np.asarray(starts, np.int32), mirror=mir,
                n=n, centres=centres, truth=truth,
                params=dict(DEFAULTS, grid=grid, n_views=n_views, extent_mm=extent_mm, **params))


def single_cases(head: Head, n_out=3, stride=16):
    """The single cases of the issue, by name -> case; what each shows is asserted by check_single."""
    out = {}
    # a flipped view: the camera's x axis turned round (det -1); its maps are stored under the mirror joints
    c = make_case(head, n_out, (3,), seed=11, stride=stride, flip_rows=(1,))
    out['flipped-view'] = c
    c = make_case(head, n_out, (3, 2), seed=12, stride=stride)
    c['xy'][int(c['rows'][0]), 1, 0, head.side - 1] = np.nan    # person 0, joint 1: one row less (mirror: identity views)
    out['nan-map'] = c
    c = make_case(head, n_out, (3, 2), seed=13, stride=stride)
    c['records'][int(c['rows'][4])]['cam_loc'][1] = np.inf      # person 1: one row less for every joint
    out['non-finite-record'] = c
    c = make_case(head, n_out, (3,), seed=14, stride=stride)
    c['rows'] = np.array([c['rows'][0], -1, c['rows'][1], c['n'], c['rows'][2]], np.int32)
    c['starts'] = np.array([0, 5], np.int32)
    out['row-index-outside'] = c
    c = make_case(head, n_out, (3,), seed=15, stride=stride)    # a fourth camera 250 mm from the joints, looking across the cube
    near_cam = c['truth'][0].mean(axis=0) + np.array([250.0, 40.0, 10.0])
    spare = int(np.setdiff1d(np.arange(c['n']), c['rows'])[0])
    c['records'][spare] = ring_records([0.0], head.side * stride)[0]
    c['records'][spare]['rot_to_world'] = look_at(near_cam, c['truth'][0].mean(axis=0)).astype(np.float32).reshape(-1)
    c['records'][spare]['cam_loc'] = near_cam.astype(np.float32)
    c['rows'], c['starts'] = np.append(c['rows'], spare).astype(np.int32), np.array([0, 4], np.int32)
    out['behind-a-camera'] = c
    out['outside-the-map'] = make_case(head, n_out, (3,), seed=16, stride=stride, extent_mm=4000.0)
    c = make_case(head, n_out, (3, 3), seed=17, stride=stride)
    c['centres'][0, 1, 2] = np.nan
    c['centres'][1, 0, 0] = np.inf
    out['nan-centre'] = c
    return out


def check_single(name, c, ref):
    """What each single case is there to show, on the restatement's outputs (which the code under test is held to)."""
    n_rows, n_out = ref['n_rows'], ref['n_rows'].shape[1]
    if name == 'flipped-view':
        assert (n_rows == 3).all() and (c['mirror'] != np.arange(n_out)).any()
    elif name == 'nan-map':
        want = np.array([[3] * n_out, [2] * n_out])
        want[0, 1] = 2
        assert np.array_equal(n_rows, want)
    elif name == 'non-finite-record':
        assert np.array_equal(n_rows, np.array([[3] * n_out, [1] * n_out]))
    elif name == 'row-index-outside':
        assert (n_rows == 3).all()
    elif name == 'behind-a-camera':
        assert (n_rows == 4).all() and c['behind'] > 0
    elif name == 'outside-the-map':
        assert (n_rows == 3).all() and c['outside'] > 0
    elif name == 'nan-centre':
        want = np.full((2, n_out), 3)
        want[0, 1] = want[1, 0] = 0
        assert np.array_equal(n_rows, want) and np.isnan(ref['points'][0, 1]).all() and np.isnan(ref['points'][1, 0]).all()
    else:
        raise KeyError(name)


def count_floor_points(c):
    """For the cases about points behind a camera or outside a map: how many (row, point) pairs of person 0, joint 0 take the
    floor for either reason -> (behind, outside)."""
    head, par = c['head'], c['params']
    g = -par['extent_mm'] / 2 + np.arange(par['grid']) * (par['extent_mm'] / (par['grid'] - 1))
    pts = c['centres'][0, 0].astype(np.float64) + np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)
    behind = outside = 0
    for i in c['rows'][c['starts'][0]:c['starts'][1]]:
        if not 0 <= i < c['n']:
            continue
        rec = c['records'][i]
        cam = (pts - rec['cam_loc'].astype(np.float64)) @ rec['rot_to_world'].astype(np.float64).reshape(3, 3)
        front = cam[:, 2] > par['near_mm']
        f = cells_of(head, rec, pts[front])
        behind += int((~front).sum())
        outside += int(((f < 0) | (f > head.side - 1)).any(axis=1).sum())
    return behind, outside
