"""Persons followed through several calibrated cameras over video, without a GPU: the covariance of the triangulated joint on
known answers and against the fp64 restatement (tests/world_follow_ref.py), the step gate of the affinity, the person steps, all
three on the kernels' own per-thread code compiled for the host, the restated chain on a synthetic rig (ids through a
crossing, a stream cut into calls), and the new C symbols in header, bindings and library."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from metro_pose3d_amd import ModelSpec, _lib, frames as FR, heads as MH
from tests import follow_tracks_ref as FT
from tests import match_views_ref as MR
from tests import track_smoothing_ref as TS
from tests import triangulation_ref as TR
from tests import world_follow_ref as WR
from tests.helpers import compile_for_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC = ModelSpec(50, 32, 'h36m')
SK = SPEC.skeleton
STEP_CASES = WR.person_steps_cases()


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    """The per-thread code of the three launches is __host__ __device__: the sources compiled for the host, one call where the
    launch has one thread."""
    tmp = tmp_path_factory.mktemp('host_world_follow')
    dll = compile_for_host(tmp, 'host_world_follow', ['triangulate.hip', 'match_views.hip', 'world_tracks.hip'], '''
#include <vector>
extern "C" void host_triangulate_cov(const float* coords01, const float* cov01, const MetroPlacement* rec, int m, const int* rows,
                                     int n_rows, const int* starts, int n_persons, const MetroSpec* spec, const int* mirror,
                                     int weights, double min_det, float* points, int* n_rays, float* residual, float* cov) {
    metro::TriArgs a = metro::make_tri_args(coords01, cov01, rec, m, rows, n_rows, starts, n_persons, *spec, mirror, weights,
                                            min_det, points, n_rays, residual);
    a.cov = cov;
    for (int idx = 0; idx < n_persons * spec->n_joints_out; ++idx) {
        if (cov) metro::triangulate_joint_t<true>(a, idx);
        else metro::triangulate_joint(a, idx);
    }
}
extern "C" void host_affinity_steps(const float* coords01, const float* cov01, const MetroPlacement* rec, const MetroSpec* spec,
                                    const int* mirror, const int* frame_index, const int* step_index, int n, int n_views,
                                    int weights, double min_sin2, double clip_mm, int min_pairs, float* cost, int* n_pairs) {
    metro::MatchArgs a = metro::make_match_args(coords01, cov01, rec, *spec, mirror, frame_index, n, n_views, weights, min_sin2,
                                                clip_mm, min_pairs, cost, n_pairs);
    a.step_index = step_index;
    for (int idx = 0; idx < n * n; ++idx) metro::view_affinity_entry(a, idx);
}
extern "C" void host_person_steps(const int* rows, int n_rows, const int* starts, const int* n_persons, int n, int n_views,
                                  const int* box_step, int n_boxes, const double* step_times, int n_steps, int* person_step,
                                  double* person_times, int* step_rows, int* step_starts) {
    metro::PersonStepsArgs a;
    a.rows = rows; a.starts = starts; a.n_persons = n_persons; a.box_step = box_step; a.step_times = step_times;
    a.person_step = person_step; a.person_times = person_times; a.step_rows = step_rows; a.step_starts = step_starts;
    a.n = n; a.n_rows = n_rows; a.n_views = n_views; a.n_boxes = n_boxes; a.n_steps = n_steps;
    std::vector<int> step(metro::PERSON_STEPS_THREADS, -99);
    for (int p = 0; p < n; ++p) metro::person_steps_assign(a, step.data(), p);
    for (int p = 0; p < n; ++p) metro::person_steps_rank(a, step.data(), p);
    for (int t = 0; t < metro::PERSON_STEPS_THREADS; ++t) metro::person_steps_starts(a, step.data(), t, metro::PERSON_STEPS_THREADS);
}
''')
    P = C.c_void_p
    tri, aff, stp = dll.host_triangulate_cov, dll.host_affinity_steps, dll.host_person_steps
    tri.restype = aff.restype = stp.restype = None
    tri.argtypes = [P] * 3 + [C.c_int, P, C.c_int, P, C.c_int, C.POINTER(_lib.MetroSpec), P, C.c_int, C.c_double] + [P] * 4
    aff.argtypes = [P] * 3 + [C.POINTER(_lib.MetroSpec), P, P, P, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, P, P]
    stp.argtypes = [P, C.c_int, P, P, C.c_int, C.c_int, P, C.c_int, P, C.c_int, P, P, P, P]
    ptr = lambda a: P(a.ctypes.data if a is not None else 0)
    mirror = np.asarray(SK.out_mirror, np.int32)

    def triangulate(c, with_cov=True):
        n_persons, n_out = len(c['starts']) - 1, SK.n_out
        rec = np.ascontiguousarray(FR.pack_placements(c['places']))
        points = np.full((n_persons, n_out, 3), -7.0, np.float32)
        n_rays = np.full((n_persons, n_out), -7, np.int32)
        residual = np.full((n_persons, n_out), -7.0, np.float32)
        cov = np.full((n_persons, n_out, 9), -7.0, np.float32) if with_cov else None
        cs = SPEC.to_c(1)
        tri(ptr(c['coords01']), ptr(c['cov01']), ptr(rec), len(c['coords01']), ptr(c['rows']), len(c['rows']), ptr(c['starts']),
            n_persons, C.byref(cs), ptr(mirror), MH.TRI_WEIGHTS[c['weights']], TR.min_det(c['min_angle_deg']), ptr(points),
            ptr(n_rays), ptr(residual), ptr(cov))
        return points, n_rays, residual, cov

    def affinity(c, step_index):
        n = len(c['fi'])
        rec = np.ascontiguousarray(FR.pack_placements(c['places']))
        fi = np.ascontiguousarray(c['fi'], np.int32)
        si = None if step_index is None else np.ascontiguousarray(step_index, np.int32)
        cost, n_pairs = np.full((n, n), -7.0, np.float32), np.full((n, n), -7, np.int32)
        cs = SPEC.to_c(1)
        aff(ptr(c['coords01']), ptr(c['cov01']), ptr(rec), C.byref(cs), ptr(mirror), ptr(fi), ptr(si), n, c['n_views'],
            MH.TRI_WEIGHTS[c['weights']], float(np.sin(np.radians(c['min_angle_deg'])) ** 2), c['clip_mm'], MR.min_pairs_of(c, SPEC),
            ptr(cost), ptr(n_pairs))
        return cost, n_pairs

    def steps(c):
        n, n_steps = c['n'], len(c['step_times'])
        count = np.asarray([c['n_persons']], np.int32)
        person_step, step_rows, step_starts = (np.full(k, WR.SENTINEL, np.int32) for k in (n, n, n_steps + 1))
        person_times = np.full(n, float(WR.SENTINEL))
        stp(ptr(c['rows']), len(c['rows']), ptr(c['starts']), ptr(count), n, c['n_views'], ptr(c['box_step']), len(c['box_step']),
            ptr(np.ascontiguousarray(c['step_times'], np.float64)), n_steps, ptr(person_step), ptr(person_times), ptr(step_rows),
            ptr(step_starts))
        return person_step, person_times, step_rows, step_starts
    return triangulate, affinity, steps


# ---- covariance of the triangulated joint: known answers -----------------------------------------------------------------------

def _exact_rays(directions, point=(100.0, -200.0, 1500.0), depth=1000.0, var_px=1e-4, weights='covariance'):
    """One person whose every joint is seen by one ray per direction, all meeting exactly at `point` from `depth` mm away:
    hand-made records with inv_intrinsics = I shifted so that coords01 = 0 looks along the camera's z, which rot_to_world turns
    into the direction.  var_px [k]: the isotropic pixel variance of each ray (with inv_intrinsics[0] = 1: sigma^2 of the ray),
    so the pass-2 weight is 1 / (var_px depth^2)."""
    k = len(directions)
    lrc, half = TR.pixel_scale(SPEC)
    inv_k = np.array([[1, 0, -half], [0, 1, -half], [0, 0, 1]], np.float32)
    rot = np.zeros((k, 3, 3), np.float32)
    loc = np.zeros((k, 3), np.float32)
    for i, d in enumerate(np.asarray(directions, np.float64)):
        x = np.cross(d, [0.3, 0.5, 0.8])
        x /= np.linalg.norm(x)
        rot[i] = np.stack([x, np.cross(d, x), d], axis=1)             # columns: the camera's axes in the world, det +1
        loc[i] = np.asarray(point) - depth * d
    assert (np.linalg.det(rot.astype(np.float64)) > 0).all()
    eye = np.tile(np.eye(3, dtype=np.float32), (k, 1, 1))
    places = FR.PlacementParams(np.zeros(k, np.int32), np.tile(inv_k, (k, 1, 1)), eye.copy(), rot, loc, eye.copy(), eye.copy(),
                                np.zeros((k, 5), np.float32))
    var = np.broadcast_to(np.asarray(var_px, np.float64).reshape(-1, 1), (k, SK.n_head))
    return TR.case(np.zeros((k, SK.n_head, 3), np.float32), TR.cov01_for(var, SPEC, (k, SK.n_head)), places, np.arange(k), [0, k],
                   weights)


def test_covariance_of_two_and_three_orthogonal_rays(host):
    """Exact rays of equal weight w.  Along x and y: A = w diag(1, 1, 2), Cov = diag(1/w, 1/w, 1/(2w)).  Three mutually orthogonal
    rays: A = 2 w I, Cov = I / (2w).  w = 1 / (1e-4 x 1000^2) = 1e-2 mm^-2 up to the fp32 rounding of the variance."""
    w = 1.0 / (float(np.float32(1e-4 / TR.pixel_scale(SPEC)[0] ** 2)) * TR.pixel_scale(SPEC)[0] ** 2 * 1000.0 ** 2)
    for dirs, want in (([[1, 0, 0], [0, 1, 0]], np.diag([1 / w, 1 / w, 1 / (2 * w)])),
                       ([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.eye(3) / (2 * w))):
        c = _exact_rays(dirs)
        points, n_rays, _, cov = host[0](c)
        assert (n_rays == len(dirs)).all() and np.abs(points - np.array([100.0, -200.0, 1500.0])).max() <= TR.KNOWN_ANSWER_MM
        worst = np.abs(cov.reshape(-1, 3, 3) - want).max() / np.abs(want).max()
        print(f'{len(dirs)} rays: Cov[0] = {cov[0, 0].tolist()}, worst deviation {worst:.2e} of the largest entry')
        assert worst <= 1e-5                               # fp32 outputs and fp32 record fields: a few 1e-7
        WR.compare_covariance(cov, WR.covariance(c, SPEC)[0], points)


def test_covariance_grows_along_the_uncertain_cameras_lateral_directions_only(host):
    """Rays along x and y; the second camera (along y) declares 100 x the variance.  Its ray constrains x and z: Cov_xx grows
    from 1/w to 100/w, Cov_yy (fixed by the first ray alone) stays 1/w, Cov_zz goes from 1/(2w) to 1/(1.01 w)."""
    base = host[0](_exact_rays([[1, 0, 0], [0, 1, 0]]))[3][0, 0].reshape(3, 3).astype(np.float64)
    cov = host[0](_exact_rays([[1, 0, 0], [0, 1, 0]], var_px=[1e-4, 1e-2]))[3][0, 0].reshape(3, 3).astype(np.float64)
    w = 1.0 / base[0, 0]
    assert np.isclose(cov[0, 0], 100 / w, rtol=1e-5) and np.isclose(cov[1, 1], base[1, 1], rtol=1e-5)
    assert np.isclose(cov[2, 2], 1 / (1.01 * w), rtol=1e-5)
    assert np.abs(cov - np.diag(np.diag(cov))).max() <= 1e-5 * cov.max()


def test_uniform_covariance_of_exactly_meeting_rays_is_zero_and_the_smoother_uses_the_row(host):
    """Uniform weights: s^2 is 0 for rays that meet exactly, so the block is 0 (never negative or NaN); the smoother's
    sigma_floor keeps R positive definite and the row enters the update (used == 1)."""
    c = _exact_rays([[1, 0, 0], [0, 1, 0]], point=(0.0, 0.0, 0.0), weights='uniform')
    c['places'].cam_loc[:] = [[-1000, 0, 0], [0, -1000, 0]]            # exact in fp32: the rays meet exactly
    points, _, residual, cov = host[0](c)
    assert (residual == 0).all() and (cov == 0).all() and (points == 0).all()
    WR.compare_covariance(cov, WR.covariance(c, SPEC)[0], points)
    used = TS.smooth_tracks(points, cov, [0.0], [0], [0, 1], 'filter', 'covariance')[3]
    assert (used[0] == 1).all()


# ---- covariance against the restatement, on the cases of the triangulation tests ---------------------------------------------

@pytest.mark.parametrize('name', list(TR.CASES))
@pytest.mark.parametrize('weights', ['uniform', 'covariance'])
def test_covariance_on_the_host_matches_the_restatement(host, name, weights):
    c = TR.CASES[name](SPEC, weights)
    points, n_rays, residual, cov = host[0](c)
    plain = host[0](c, with_cov=False)
    for g, w in zip((points, n_rays, residual), plain):
        assert np.array_equal(g, w, equal_nan=True), 'points, n_rays and residual are the plain entry\'s, bit for bit'
    TR.compare((points, n_rays, residual), TR.expected(c, SPEC), TR.PARITY_MM)
    want, det = WR.covariance(c, SPEC)
    solved = ~np.isnan(points).any(axis=-1)
    assert np.array_equal(~np.isnan(det), solved) and (det[solved] >= TR.min_det(c['min_angle_deg'])).all()
    worst = WR.compare_covariance(cov, want, points)
    sym = cov.reshape(-1, 3, 3)
    assert np.array_equal(sym, sym.transpose(0, 2, 1), equal_nan=True)
    print(f'{name}, {weights}: {int(solved.sum())} blocks, worst deviation {worst:.2e} of the largest entry, smallest det A~ '
          f'{np.nanmin(det) if solved.any() else float("nan"):.3g}')
    if name == 'ragged':
        assert solved[:3].all() and not solved[3].any() and (cov[:3].reshape(-1, 3, 3)[:, [0, 1, 2], [0, 1, 2]] > 0).all()


# ---- the step gate ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('weights', ['uniform', 'covariance'])
def test_gate_leaves_same_step_pairs_alone_and_cuts_the_others(host, weights):
    c = MR.CASES['scrambled'](SPEC, weights)
    n = len(c['fi'])
    plain = host[1](c, None)
    MR.compare(plain, MR.expected(c, SPEC), MR.PARITY_MM)
    for same in (np.zeros(n, np.int32), np.full(n, 5, np.int32)):
        got = host[1](c, same)
        assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
    step = (np.arange(n) % 2).astype(np.int32)
    got = host[1](c, step)
    want = WR.gated(*plain, step)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    MR.compare(got, WR.gated(*MR.expected(c, SPEC), step), MR.PARITY_MM)
    other = step[:, None] != step[None, :]
    assert np.isposinf(got[0][other]).all() and (got[1][other] == 0).all() and np.isfinite(got[0][~other]).any()


def test_clusters_of_the_gated_matrix_never_span_two_steps(host):
    """Two persons standing still over two exposures: cameras 0 and 1 of a 4-camera rig see them at step 0, cameras 2 and 3 at
    step 1, all with exact projections of the same joints.  Ungated, the four boxes of a person cost about 0 against each other
    and cluster into one person across the steps; gated, every cluster lies in one step."""
    s = MR.rig_scene([0, 70, 140, 230], 2, SPEC, seed=2)
    n = len(s['fi'])
    c = MR.case(s, SPEC, 'covariance')
    step = (c['fi'] >= 2).astype(np.int32)
    plain, got = host[1](c, None), host[1](c, step)
    across = (c['pi'][:, None] == c['pi'][None, :]) & (step[:, None] != step[None, :])
    assert plain[0][across].max() <= MR.KNOWN_ANSWER_MM, 'ungated, the same person across the steps costs about 0'
    labels = MR.cluster(plain[0], MR.MAX_COST_MM)[0]
    assert any(len(set(step[labels == p])) == 2 for p in set(labels)), 'ungated clusters do span the steps'
    labels, n_persons, rows, starts = MR.cluster(got[0], MR.MAX_COST_MM)
    assert n_persons == 4 and all(len(set(step[labels == p])) == 1 for p in range(n_persons))
    assert np.array_equal(labels, c['pi'] + 2 * step)
    # ... and the ungated clusters take the smallest step in the person steps
    ungated = MR.cluster(plain[0], MR.MAX_COST_MM)
    c_steps = dict(rows=ungated[2], starts=ungated[3], n_persons=ungated[1], n=n, n_views=1, box_step=step,
                   step_times=np.array([0.0, 0.25]))
    out = host[2](c_steps)
    WR.compare_person_steps(out, WR.person_steps(**c_steps))
    spanning = [p for p in range(ungated[1]) if len(set(step[ungated[0] == p])) == 2]
    assert spanning and all(out[0][p] == 0 for p in spanning)


# ---- the person steps ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(STEP_CASES))
def test_person_steps_on_the_host_match_the_restatement(host, name):
    c = STEP_CASES[name]
    got = host[2](c)
    want = WR.person_steps(**c)
    WR.compare_person_steps(got, want)
    person_step, person_times, step_rows, step_starts = got
    n_steps = len(c['step_times'])
    with_step = person_step >= 0
    assert step_starts[0] == 0 and step_starts[n_steps] == with_step.sum() and (np.diff(step_starts) >= 0).all()
    assert (step_rows[with_step.sum():] == -1).all() and sorted(step_rows[:with_step.sum()]) == list(np.flatnonzero(with_step))
    assert np.array_equal(np.isnan(person_times), ~with_step) and (person_step[c['n_persons']:] == -1).all()
    assert np.array_equal(person_times[with_step], c['step_times'][person_step[with_step]])
    if name == 'descending':
        assert step_rows.tolist()[:4] == [3, 2, 1, 0] and person_step.tolist()[:4] == [3, 2, 1, 0], 'the sort permutes'
    elif name == 'empty-step':
        assert step_starts.tolist() == [0, 1, 1, 2]
    elif name == 'ungated':
        assert person_step.tolist()[:2] == [1, 0] and step_rows.tolist()[:2] == [1, 0]
    elif name == 'rows-out-of-range':
        assert person_step.tolist() == [0, 1, -1, -1]
    elif name == 'steps-out-of-range':
        assert person_step.tolist() == [-1, 1, -1, -1] and step_starts.tolist() == [0, 0, 1]
    elif name in ('count-0', 'singles'):
        assert (person_step == -1).all() and (step_starts == 0).all() and (step_rows == -1).all()
    elif name == 'count-below-n-garbage':
        assert person_step.tolist() == [0, 0, -1, -1, -1, -1]


# ---- the restated chain on a synthetic rig ------------------------------------------------------------------------------------

def _person_of(s, boxes, r):
    """The true (step, person) of every person the chain found, from its lowest box."""
    lowest = [int(np.flatnonzero(r['person_index'] == p)[0]) for p in range(r['n_persons'])]
    return s['step'][boxes][lowest], s['pi'][boxes][lowest]


def test_two_persons_keep_their_ids_through_a_crossing():
    s, calls = WR.walking_in_calls(8)
    (boxes, r), = calls
    assert len(boxes) == 64 and r['n_persons'] == 16
    step, person = _person_of(s, boxes, r)
    assert np.array_equal(r['person_index'], [np.flatnonzero((step == t) & (person == p))[0] for t, p in zip(s['step'], s['pi'])])
    assert np.array_equal(r['person_step'][:16], step) and (r['person_step'][16:] == -1).all() and (r['n_rays'][:16] == 4).all()
    truth = s['truth'][step, person]
    err = np.abs(r['points'][:16] - truth).max()
    a = r['assoc']
    print(f"worst joint {err:.2e} mm; pick margin {a['margin_pick']:.3g} mm, gate margin {a['margin_gate']:.3g} mm")
    assert err <= TR.KNOWN_ANSWER_MM
    ids = a['track_id'][:16]
    for p in (0, 1):
        assert len(set(ids[person == p].tolist())) == 1 and ids[person == p][0] >= 0
    assert ids[person == 0][0] != ids[person == 1][0] and a['n_new'] == 2 and a['n_dropped'] == 0 and (a['track_id'][16:] == -1).all()
    centres = truth.mean(axis=1)
    gap = [centres[(step == t) & (person == 0)][0, 0] - centres[(step == t) & (person == 1)][0, 0] for t in range(8)]
    assert gap[3] < 0 < gap[4] and abs(gap[3]) < 150 and abs(gap[4]) < 150, 'the persons pass each other between steps 3 and 4'
    # every decision at least 1e-2 mm from flipping: the 1e-3 mm allowed on a cost cannot change one
    assert a['margin_pick'] >= FT.MARGIN_MM and a['margin_gate'] >= FT.MARGIN_MM
    # the smoothing restatement used every row, and its state agrees with the association's working state
    used, state = r['smoothed'][3], r['smoothed'][4]
    assert (used[:16] == 1).all()
    live = ~np.isnan(a['working'][..., 27])
    assert np.array_equal(np.isnan(state[..., 27]), ~live)
    scale = np.abs(a['working'][live][:, :27]).max(axis=1, keepdims=True)
    assert (np.abs(state[live][:, :27] - a['working'][live][:, :27]) / scale).max() <= FT.STATE_REL


@pytest.mark.parametrize('steps_per_call', [1, 3])
def test_stream_cut_into_calls_gives_the_ids_and_states_of_one_call(steps_per_call):
    s, ((boxes, whole),) = WR.walking_in_calls(8)
    _, calls = WR.walking_in_calls(steps_per_call)
    assert len(calls) == -(-8 // steps_per_call)
    ids = {}
    for part, r in calls:
        step, person = _person_of(s, part, r)
        for t, p, i in zip(step, person, r['assoc']['track_id'][:r['n_persons']]):
            ids[int(t), int(p)] = int(i)
    step, person = _person_of(s, boxes, whole)
    want = {(int(t), int(p)): int(i) for t, p, i in zip(step, person, whole['assoc']['track_id'][:16])}
    assert ids == want
    last = calls[-1][1]['table']
    assert np.array_equal(last[1], whole['table'][1]) and int(last[2][0]) == int(whole['table'][2][0])
    for slot in np.flatnonzero(last[1] >= 0):
        assert np.array_equal(last[0][slot], whole['table'][0][slot]), 'per id, the state bit for bit'


# ---- the surface ----------------------------------------------------------------------------------------------------------

def test_python_surface():
    import metro_pose3d_amd
    assert metro_pose3d_amd.follow_world_poses_in_frames is FR.follow_world_poses_in_frames
    assert 'follow_world_poses_in_frames' in metro_pose3d_amd.__all__
    sig = inspect.signature(FR.follow_world_poses_in_frames)
    assert list(sig.parameters)[:8] == ['frames', 'boxes', 'model_path', 'cameras', 'frame_index', 'timestamps', 'tracks', 'capacity']
    d = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    match = {k: p.default for k, p in inspect.signature(FR.match_poses_in_frames).parameters.items()}
    follow = {k: p.default for k, p in inspect.signature(FR.follow_poses_in_frames).parameters.items()}
    assert (d['match_max_cost_mm'], d['match_clip_mm'], d['match_min_joints']) == (match['max_cost_mm'], match['clip_mm'], match['min_joints'])
    for k in ('weights', 'min_angle_deg'):
        assert d[k] == match[k]
    for k in ('capacity', 'max_cost_mm', 'clip_mm', 'min_joints', 'max_age_s', 'mode', 'measurement', 'accel_psd', 'sigma_floor_mm',
              'cov_scale', 'initial_speed_mm_s', 'gate'):
        assert d[k] == follow[k], k
    assert FR.FollowedWorldPoses._fields == ('person_index', 'cost', 'n_pairs', 'world', 'world_covariance', 'person_step', 'track_index',
                                            'track_id', 'track_cost', 'n_new', 'n_dropped', 'tracks', 'smoothed')
    assert FR.SmoothedWorldPoses._fields == ('poses', 'velocity', 'covariance', 'used', 'state')
    assert list(inspect.signature(MH.view_affinity_steps).parameters)[:6] == ['coords01', 'cov01', 'places', 'frame_index', 'step_index', 'spec']
    assert 'step_index' not in inspect.signature(MH.view_affinity).parameters
    assert inspect.signature(MH.triangulate_joints).parameters['return_covariance'].default is False
    assert list(inspect.signature(MH.person_steps).parameters) == ['rows', 'starts', 'n_persons', 'box_step', 'step_times', 'n_views']


def test_new_symbols_in_header_bindings_and_library(lib):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'metro_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(metro_[a-z0-9_]+)\s*\(', text))
    for name, n_args in (('metro_view_affinity_steps', 16), ('metro_triangulate_joints_cov', 17), ('metro_person_steps', 15)):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
        params = re.search(r'\b' + name + r'\s*\(([^)]*)\)', text).group(1)
        assert len(_lib.SIGNATURES[name][1]) == params.count(',') + 1 == n_args
    assert lib.metro_abi_version() == 8                    # the ABI is additive
    from metro_pose3d_amd import build
    assert 'world_tracks.hip' in build.SOURCES


def test_c_entries_reject_bad_arguments(lib):
    """Every return below comes before any launch: no device is needed."""
    cs = SPEC.to_c(_lib.METRO_PREC_F16)
    p, md = C.c_void_p(256), TR.min_det(2.0)
    tri = [p, p, p, 4, p, 4, p, 2, C.byref(cs), p, _lib.METRO_TRI_COVARIANCE, md, p, p, p, p, None]
    assert lib.metro_triangulate_joints_cov(*tri[:15], None, None) == -1 and b'cov_out' in lib.metro_last_error()
    assert lib.metro_triangulate_joints_cov(*tri[:10], 7, *tri[11:]) == -1 and b'weights' in lib.metro_last_error()
    assert lib.metro_triangulate_joints_cov(*tri[:7], 0, *tri[8:15], None, None) == 0          # no persons: nothing to launch
    aff = [p, p, p, C.byref(cs), p, p, p, 4, 1, _lib.METRO_TRI_COVARIANCE, 0.5, 500.0, 9, p, p, None]
    assert lib.metro_view_affinity_steps(*aff[:6], None, *aff[7:]) == -1 and b'step_index' in lib.metro_last_error()
    assert lib.metro_view_affinity_steps(*aff[:7], 129, *aff[8:]) == -1 and b'at most' in lib.metro_last_error()
    assert lib.metro_view_affinity_steps(*aff[:7], 0, *aff[8:]) == 0
    stp = [p, 4, p, p, 4, 1, p, 4, p, 2, p, p, p, p, None]
    assert lib.metro_person_steps(*stp[:4], 129, *stp[5:]) == -1 and b'at most' in lib.metro_last_error()
    assert lib.metro_person_steps(*stp[:4], -1, *stp[5:]) == -1 and b'negative' in lib.metro_last_error()
    assert lib.metro_person_steps(*stp[:5], 0, *stp[6:]) == -1 and b'views' in lib.metro_last_error()
    for k in (0, 2, 3, 6, 8, 10, 11, 12, 13):
        a = list(stp)
        a[k] = None
        assert lib.metro_person_steps(*a) == -1 and b'person_steps' in lib.metro_last_error(), k
    assert lib.metro_person_steps(*stp[:4], 0, *stp[5:]) == 0
