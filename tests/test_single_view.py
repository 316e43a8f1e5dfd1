"""A person only one camera sees keeps feeding its world track, without a GPU: the person steps from labels, the rays and the
association walk with ray rows, each on the kernels' own __host__ __device__ code compiled for the host, against known answers
and the fp64 restatement (tests/single_view_ref.py); what the feature is for, on the restatement (two of three cameras lose a
person for 1.5 s); a stream cut into calls; and the new C symbols and Python surface."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from metro_pose3d_amd import ModelSpec, _lib, frames as FR, heads as MH
from tests import assign_tracks_ref as AR
from tests import follow_tracks_ref as FT
from tests import single_view_ref as SV
from tests import track_smoothing_ref as TS
from tests import triangulation_ref as TR
from tests import world_follow_ref as WR
from tests.assoc_host import NO_RAY_ROW_CASES, assert_ray_walk_is_the_plain_walk, compile_walk, ptr, without_ray_rows
from tests.test_world_follow import _exact_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC = ModelSpec(50, 32, 'h36m')
SK = SPEC.skeleton
LABEL_CASES = SV.labels_cases()
RULES = ('greedy', 'optimal')


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    """The per-thread code of the three launches compiled for the host and run by one thread: person_steps_labels_kernel's three
    steps, person_ray per (person, joint), and associate_tracks.hip's walk with ray rows, the function its kernels run
    (tests/assoc_host.py, which also brings smooth_tracks.hip's per-joint function for the state the smoothing launch leaves on
    what the walk wrote)."""
    tmp = tmp_path_factory.mktemp('host_single_view')
    dll, associate = compile_walk(tmp, 'host_single_view', ['world_tracks.hip', 'person_rays.hip'], '''
#include <vector>
extern "C" void host_person_steps_labels(const int* person_index, const int* n_persons, int n, const int* box_step, int n_boxes,
                                         const double* step_times, int n_steps, int* person_step, double* person_times,
                                         int* step_rows, int* step_starts, int* single_box) {
    metro::PersonLabelsArgs a;
    a.rows = nullptr; a.starts = nullptr; a.n_persons = n_persons; a.box_step = box_step; a.step_times = step_times;
    a.person_step = person_step; a.person_times = person_times; a.step_rows = step_rows; a.step_starts = step_starts;
    a.n = n; a.n_rows = 0; a.n_views = 1; a.n_boxes = n_boxes; a.n_steps = n_steps;
    a.person_index = person_index; a.single_box = single_box;
    std::vector<int> step(metro::PERSON_STEPS_THREADS, -99);
    for (int p = 0; p < n; ++p) metro::person_labels_assign(a, step.data(), p);
    for (int p = 0; p < n; ++p) metro::person_steps_rank(a, step.data(), p);
    for (int t = 0; t < metro::PERSON_STEPS_THREADS; ++t) metro::person_steps_starts(a, step.data(), t, metro::PERSON_STEPS_THREADS);
}
extern "C" void host_person_rays(const float* coords01, const float* cov01, const MetroPlacement* rec, int m, const MetroSpec* spec,
                                 const int* mirror, int weights, const int* single_box, int n, int n_views, double* rays) {
    const metro::PersonRaysArgs a = metro::make_person_rays_args(coords01, cov01, rec, m, *spec, mirror, weights, single_box, n,
                                                                 n_views, rays);
    for (int idx = 0; idx < n * spec->n_joints_out; ++idx) metro::person_ray(a, idx);
}
''')
    P = C.c_void_p
    stp, ray = dll.host_person_steps_labels, dll.host_person_rays
    stp.restype = ray.restype = None
    stp.argtypes = [P, P, C.c_int, P, C.c_int, P, C.c_int, P, P, P, P, P]
    ray.argtypes = [P, P, P, C.c_int, C.POINTER(_lib.MetroSpec), P, C.c_int, P, C.c_int, C.c_int, P]

    def labels(c):
        n, n_steps = c['n'], len(c['step_times'])
        count = np.asarray([c['n_persons']], np.int32)
        person_step, step_rows, step_starts, single = (np.full(k, SV.SENTINEL, np.int32) for k in (n, n, n_steps + 1, n))
        person_times = np.full(n, float(SV.SENTINEL))
        stp(ptr(c['person_index']), ptr(count), n, ptr(c['box_step']), len(c['box_step']),
            ptr(np.ascontiguousarray(c['step_times'], np.float64)), n_steps, ptr(person_step), ptr(person_times), ptr(step_rows),
            ptr(step_starts), ptr(single))
        return person_step, person_times, step_rows, step_starts, single

    def rays(c, spec=SPEC):
        n, n_out = len(c['single_box']), spec.skeleton.n_out
        rec = np.ascontiguousarray(FR.pack_placements(c['places']))
        out = np.full((n, n_out, 8), float(SV.SENTINEL))
        cs = spec.to_c(1)
        mirror = np.asarray(spec.skeleton.out_mirror, np.int32)
        single = np.ascontiguousarray(c['single_box'], np.int32)
        ray(ptr(c['coords01']), ptr(c['cov01']), ptr(rec), len(c['coords01']), C.byref(cs), ptr(mirror), MH.TRI_WEIGHTS[c['weights']],
            ptr(single), n, c['n_views'], ptr(out))
        return out

    return labels, rays, lambda c, assignment='greedy': associate(c, assignment, ray_rows=True), associate


# ---- the person steps from labels ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(LABEL_CASES))
def test_person_steps_from_labels_on_the_host_match_the_restatement(host, name):
    c = LABEL_CASES[name]
    got, want = host[0](c), SV.person_steps_labels(**c)
    WR.compare_person_steps(got[:4], want[:4])
    assert np.array_equal(got[4], want[4]), (got[4], want[4])
    single = got[4]
    count = min(c['n_persons'], c['n'])
    assert (single[count:] == -1).all() and (got[0][count:] == -1).all()
    for p in np.flatnonzero(single >= 0):
        assert c['person_index'][single[p]] == p and (c['person_index'] == p).sum() == 1 and got[0][p] == c['box_step'][single[p]]
    if name.endswith('all-single'):
        assert (single >= 0).all() and sorted(single.tolist()) == list(range(c['n']))
    elif name.endswith('pairs') and c['n'] % 2 == 0 or name == 'n2-pair':
        assert (single == -1).all() and (got[0][:count] >= 0).all()
    elif name == 'label-out-of-range':
        assert single.tolist() == [-1, 3, 5, -1, -1, -1] and got[0].tolist() == [1, 2, 0, -1, -1, -1]
    elif name == 'step-out-of-range':
        assert single.tolist() == [-1, -1, -1, -1, -1] and got[0].tolist() == [1, -1, 0, -1, -1], 'two boxes are not one, whatever their steps'
    elif name == 'count-below-labels':
        assert single.tolist() == [0, 1, -1, -1]


@pytest.mark.parametrize('name', ['n127-mixed', 'n128-mixed', 'n128-pairs', 'n2-pair'])
def test_a_person_with_several_boxes_gets_the_step_metro_person_steps_gives(name):
    """The restatement of metro_person_steps on the cluster CSR of the same labels: equal wherever the person has a group."""
    c = LABEL_CASES[name]
    n = c['n']
    groups = [np.flatnonzero(c['person_index'] == p) for p in range(n)]
    groups = [g if len(g) > 1 else g[:0] for g in groups]                 # metro_cluster_views: a single box has an empty group
    rows = np.concatenate(groups + [np.full(n - sum(map(len, groups)), -1)]).astype(np.int32)
    starts = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
    old = WR.person_steps(rows, starts, c['n_persons'], n, 1, c['box_step'], c['step_times'])[0]
    new = SV.person_steps_labels(**c)
    several = np.array([len(g) > 1 for g in groups])
    assert several.any() and np.array_equal(old[several], new[0][several])
    assert (old[~several] == -1).all() and ((new[0][~several] >= 0) == (new[4][~several] >= 0)).all()


# ---- the rays: known answers ----------------------------------------------------------------------------------------------------

def _views_of_one_box(k, var_px=1e-4, weights='covariance', direction=(0.6, 0.0, 0.8)):
    """k views of ONE box: _exact_rays' hand-made records, all from one optical centre along `direction`."""
    c = _exact_rays([direction] * k, var_px=var_px, weights=weights)
    return dict(c, n_views=k, single_box=np.zeros(1, np.int32))


def test_one_view_gives_the_direction(host):
    c = _views_of_one_box(1)
    got = host[1](c)
    assert np.abs(got[0, :, 3:6] - [0.6, 0.0, 0.8]).max() <= 1e-6 and (got[0, :, 7] == 1).all()     # fp32 rot_to_world
    assert np.array_equal(got[0, :, :3], np.tile(c['places'].cam_loc[0].astype(np.float64), (SK.n_out, 1)))
    SV.compare_rays(got, SV.person_rays(c, SPEC))


def test_a_flipped_view_uses_the_mirror_joint(host):
    c = _views_of_one_box(2, weights='uniform')
    c['places'].rot_to_world[1][:, 0] *= -1                               # det < 0: a flipped test-time view
    lrc = TR.pixel_scale(SPEC)[0]
    c['coords01'][1, :, 0] = 0.01 * (np.arange(SK.n_head) + 1)             # every head joint somewhere else in view 1
    got = host[1](c)
    SV.compare_rays(got, SV.person_rays(c, SPEC))
    rot = c['places'].rot_to_world.astype(np.float64)
    perm, mirror = np.asarray(SK.permutation), np.asarray(SK.out_mirror)
    moved = 0
    for r in range(SK.n_out):
        def summed(head):
            d0, d1 = rot[0] @ np.array([0.0, 0.0, 1.0]), rot[1] @ np.array([float(c['coords01'][1, head, 0]) * lrc, 0.0, 1.0])
            s = d0 / np.linalg.norm(d0) + d1 / np.linalg.norm(d1)
            return s / np.linalg.norm(s)
        assert np.abs(got[0, r, 3:6] - summed(perm[mirror[r]])).max() <= 1e-9
        moved += mirror[r] != r and np.abs(got[0, r, 3:6] - summed(perm[r])).max() > 1e-4
    assert moved >= 10, 'the left and right joints of a flipped view do change places'


def test_sigma2_of_two_views_combines_as_a_parallel_sum(host):
    a, b = 1e-4, 4e-4
    got = host[1](_views_of_one_box(2, var_px=[a, b]))
    lrc = TR.pixel_scale(SPEC)[0]
    a32, b32 = (float(np.float32(v / lrc ** 2)) * lrc ** 2 for v in (a, b))
    assert np.abs(got[0, :, 6] / (1.0 / (1.0 / a32 + 1.0 / b32)) - 1.0).max() <= 1e-12 and (got[0, :, 7] == 2).all()
    assert (host[1](_views_of_one_box(2, var_px=[a, b], weights='uniform'))[0, :, 6] == 0).all()


def test_a_nan_view_is_dropped_and_two_boxes_give_no_ray(host):
    c = _views_of_one_box(2)
    c['coords01'][1] = np.nan
    got = host[1](c)
    assert (got[0, :, 7] == 1).all() and np.abs(got[0, :, 3:6] - [0.6, 0.0, 0.8]).max() <= 1e-6
    c['cov01'][0] = np.nan                                                # ... and a view without a finite weight too
    assert np.isnan(host[1](c)).all()
    # two boxes of one person: no single box, no ray
    single = host[0](dict(person_index=np.zeros(2, np.int32), n_persons=1, n=2, box_step=np.zeros(2, np.int32), step_times=[0.0]))[4]
    assert single.tolist() == [-1, -1]
    two = dict(_exact_rays([[0.6, 0.0, 0.8], [0.0, 0.6, 0.8]]), n_views=1, single_box=single)
    assert np.isnan(host[1](two)).all()
    assert not np.isnan(host[1](dict(two, single_box=np.array([1, -1], np.int32)))[0]).any()


@pytest.mark.parametrize('name', list(SV.RAY_CASES))
def test_rays_on_the_host_match_the_restatement(host, name):
    c, want = SV.rays_case_and_expected(name)
    got = host[1](c, c['spec'])
    worst = SV.compare_rays(got, want)
    have = ~np.isnan(want[..., 0])
    print(f'{name}: {int(have.sum())} of {have.size} rays, worst direction deviation {worst:.2e}')
    assert have.any() and (name == 'P1-J1-V1-covariance' or not have.all())
    assert np.abs(np.linalg.norm(got[have][:, 3:6], axis=1) - 1.0).max() <= 1e-15


# ---- cost and place: known answers ----------------------------------------------------------------------------------------------

def _one_slot(offset, direction=(0.0, 0.6, 0.8), depth=4000.0, nj=3, sigma2=1e-6, max_cost=300.0, prior=None):
    """One slot at rest whose joints lie `offset` mm off the points at `depth` on rays from one camera, seen at the step's time
    (dt = 0); one step with one ray row."""
    d = np.asarray(direction, np.float64)
    o = np.array([100.0, -50.0, 20.0])
    rng = np.random.default_rng(3)
    dirs = d + np.concatenate([np.zeros((1, 3)), rng.uniform(-0.05, 0.05, (nj - 1, 3))])
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    state, ids, next_id = FT.new_table(2, nj)
    state[0, :, :3] = o + depth * dirs + np.asarray(offset, np.float64)
    state[0, :, 6 + np.array([0, 6, 11])] = 25.0 if prior is None else np.asarray(prior, np.float64)[:, None]
    state[0, :, 6 + np.array([15, 18, 20])] = 1e4
    state[0, :, 27] = 1.0
    ids[0], next_id[0] = 0, 1
    rays = np.concatenate([np.tile(o, (nj, 1)), dirs, np.full((nj, 1), sigma2), np.ones((nj, 1))], axis=1)[None]
    return dict(FT.DEFAULTS, poses=np.full((1, nj, 3), np.nan, np.float32), cov=np.full((1, nj, 9), np.nan, np.float32), times=np.array([1.0]),
                step_rows=np.zeros(1, np.int32), step_starts=np.array([0, 1], np.int32), state=state, ids=ids, next_id=next_id,
                min_joints=1, person=np.zeros(1, int), tie=False, single_box=np.zeros(1, np.int32), rays=rays, depth_sigma=SV.DEPTH_SIGMA,
                max_cost=max_cost), dirs, o


def test_cost_is_the_distance_from_the_rays_and_blind_along_them(host):
    across = np.cross([0.0, 0.6, 0.8], [1.0, 0.0, 0.0])
    for offset, want in (((0, 0, 0), 0.0), (50.0 * np.array([1.0, 0, 0]), 50.0), (50.0 * across, 50.0)):
        c, dirs, _ = _one_slot(offset, nj=1)
        got = host[2](c)
        assert got['track_index'][0] == 0 and abs(float(got['cost'][0]) - want) <= 1e-3, (offset, got['cost'])
    c, dirs, o = _one_slot((0, 0, 0))
    c['state'][0, :, :3] += 500.0 * dirs                                   # 500 mm along each joint's own ray
    got = host[2](c)
    assert abs(float(got['cost'][0])) <= 1e-3 and np.abs(got['ray_depth'][0] - 4500.0).max() <= 1e-3


def test_behind_the_camera_costs_clip_and_is_not_placed(host):
    c, dirs, o = _one_slot((0, 0, 0), depth=-4000.0, max_cost=700.0)
    got = host[2](c)
    assert got['track_index'][0] == 0 and float(got['cost'][0]) == 600.0, 'every joint at clip_mm'
    assert np.isnan(got['ray_depth']).all() and np.isnan(got['poses']).all() and np.isnan(got['cov']).all()
    assert (got['used'] == 0).all() and np.array_equal(got['working'][0, :, :27], c['state'][0, :, :27]), 'bridged at dt = 0'
    c, _, _ = _one_slot((0, 0, 0), depth=-4000.0)
    got = host[2](c)
    assert got['track_index'][0] == -1 and got['n_unplaced'][0] == 1 and got['n_dropped'][0] == 0 and got['n_new'][0] == 0


def test_placement_is_the_foot_of_the_perpendicular_with_r_tight_across_and_wide_along(host):
    offset = np.array([30.0, -20.0, 45.0])
    c, dirs, o = _one_slot(offset, sigma2=4e-6)
    got = host[2](c)
    for j, d in enumerate(dirs):
        p = c['state'][0, j, :3]
        tau = d @ (p - o)
        foot = o + tau * d
        assert abs(float(got['ray_depth'][0, j]) - tau) <= 1e-3 and np.abs(got['poses'][0, j] - foot).max() <= 1e-3
        assert abs((p - foot) @ d) <= 1e-9 and np.linalg.norm(p - foot) > 10
        r = got['cov'][0, j].astype(np.float64).reshape(3, 3)
        assert np.array_equal(r, r.T)
        vals, vecs = np.linalg.eigh(r)
        # every entry is rounded once to fp32: |dR| <= 3 x 2^-24 of the largest entry in the Frobenius norm
        bound = 3 * 2.0 ** -24 * np.abs(r).max()
        assert abs(vals[2] - SV.DEPTH_SIGMA ** 2) <= bound and np.abs(vals[:2] - 4e-6 * tau * tau).max() <= bound, vals
        assert abs(abs(vecs[:, 2] @ d) - 1.0) <= 1e-6


def test_update_is_the_closed_form_with_a_prior_aligned_with_the_ray(host):
    """d = e_z, dt = 0, a diagonal prior diag(P_perp, P_perp, P_par): across the ray the variances combine in parallel with
    R_perp = sigma2 tau^2 + sigma_floor^2; along it the variance shrinks by P_par^2 / (P_par + depth_sigma^2 + sigma_floor^2),
    less than P_par^2 / (P_par + depth_sigma^2), and the estimate does not move along the ray at all."""
    p_perp, p_par = 400.0, 2500.0
    c, dirs, o = _one_slot((12.0, -7.0, 0.0), direction=(0.0, 0.0, 1.0), nj=1, sigma2=1e-6, prior=(p_perp, p_perp, p_par))
    c['state'][0, :, 6 + np.array([15, 18, 20])] = 1e4
    got = host[2](c)
    assert got['used'][0, 0] == 1
    r = got['cov'][0, 0].astype(np.float64).reshape(3, 3)
    assert r[0, 1] == r[0, 2] == r[1, 2] == 0.0
    x, p, t = TS.unpack_state(got['working'][0, 0])
    r_perp, r_par = r[0, 0] + 1.0, r[2, 2] + 1.0
    assert abs(p[0, 0] / (1.0 / (1.0 / p_perp + 1.0 / r_perp)) - 1.0) <= 1e-9 and abs(p[1, 1] / p[0, 0] - 1.0) <= 1e-9
    shrink = p_par - p[2, 2]
    assert abs(shrink / (p_par ** 2 / (p_par + r_par)) - 1.0) <= 1e-9 and 0 < shrink < p_par ** 2 / (p_par + SV.DEPTH_SIGMA ** 2)
    assert x[2] == c['state'][0, 0, 2], 'no innovation along the ray'
    gain = p_perp / (p_perp + r_perp)
    assert abs(x[0] - (c['state'][0, 0, 0] - gain * 12.0)) <= 1e-3 and abs(x[1] - (c['state'][0, 0, 1] + gain * 7.0)) <= 1e-3


# ---- the walk against the restatement ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('assignment', RULES)
@pytest.mark.parametrize('name', list(SV.CASES))
def test_walk_on_the_host_matches_the_restatement(host, name, assignment):
    """Integers exactly; costs, z and tau within 1e-3 mm; R within 1e-6 of its block's largest entry; the working state within
    1e-9 of the restatement's filter fed with the kernel's own fp32 z and R; and bit for bit what the smoothing kernel's own
    code leaves on the CSR and the arrays the walk wrote."""
    c = SV.case(name)
    got = host[2](c, assignment)
    want = SV.associate(c, assignment, placed=(got['poses'], got['cov']))
    SV.check_margins(want, assignment)
    worst = SV.compare(got, want, c)
    placed = ~np.isnan(got['ray_depth'])
    print(f"{name}, {assignment}: {int((c['single_box'] >= 0).sum())} ray rows, {int(placed.sum())} joints placed, "
          f"{want['n_unplaced']} unplaced; worst cost {worst[0]:.2e} mm, state {worst[1]:.2e} rel, z {worst[2]:.2e} mm, "
          f"tau {worst[3]:.2e} mm, R {worst[4]:.2e} rel; margins gate {want['margin_gate']:.3g} mm, tau {want['margin_tau']:.3g} mm")
    assert not (got['track_index'] == FT.SENTINEL).any() and not (got['ray_depth'] == FT.SENTINEL).any()
    assert np.array_equal(got['working'], got['smoothed_state'], equal_nan=True), 'the smoothing code leaves the working state, bit for bit'
    assert (got['used'][placed] == 1).all(), 'every placed joint entered the update'
    if name == 'ray-wins':
        assert got['track_index'].tolist() == [1, 0] and got['n_new'][0] == 1 and got['n_unplaced'][0] == 0
    elif name == 'point-wins':
        assert got['track_index'].tolist() == [0, -1] and got['n_unplaced'][0] == 1 and got['n_dropped'][0] == 0
    elif name == 'partial':
        assert np.flatnonzero(placed[0]).tolist() == list(range(2, 12)) and np.isnan(got['working'][0, 12:, 27]).all()
    elif name == 'exhausted':
        assert got['n_unplaced'][0] == 1 and got['n_dropped'][0] == 3 and got['n_new'][0] == 2
    elif name == 'first-sight':
        assert got['n_unplaced'][0] == 2 and got['n_new'][0] == 2 and got['n_dropped'][0] == 0
    elif name == 'T1-m1-ray-only-step':
        assert got['n_new'][0] == 1 and placed.sum() == 17 and got['n_unplaced'][0] == 0
    elif name == 'T128-m128-j1-full-table':
        assert (got['ids'] >= 0).all() and got['n_unplaced'][0] == 0 and placed.sum() == 64


@pytest.mark.parametrize('assignment', RULES)
@pytest.mark.parametrize('name', NO_RAY_ROW_CASES)
def test_walk_with_ray_rows_switched_on_and_no_ray_row_is_the_plain_walk(host, name, assignment):
    c = AR.CASES[name]()
    assert_ray_walk_is_the_plain_walk(host[2](without_ray_rows(c), assignment), host[3](c, assignment), c)


# ---- what the feature is for ---------------------------------------------------------------------------------------------------

def test_a_person_two_of_three_cameras_lose_keeps_its_id_and_stays_on_the_ray():
    """The restated walk on a 3-camera rig's stream at 30 fps in which two cameras lose the person for 45 steps.  'skip': the slot
    is too old when they return, the person comes back under a new id.  'rays': one id throughout.  And from the fifth step
    of the gap on, while 'skip' still has a bridge (max_age_s), the root's error across the seeing camera's ray is smaller."""
    truth = SV.stream_truth()
    skip, rays = SV.stream_case('skip'), SV.stream_case('rays')
    r_skip, r_rays = SV.associate(skip), SV.associate(rays)
    lo, hi = SV.STREAM_GAP
    assert r_skip['n_new'] == 2 and r_skip['track_id'][:lo].tolist() == [0] * lo and r_skip['track_id'][hi:].tolist() == [1] * (SV.STREAM_STEPS - hi)
    assert r_rays['n_new'] == 1 and r_rays['n_unplaced'] == 0 and r_rays['n_dropped'] == 0 and (r_rays['track_id'] == 0).all()
    assert not np.isnan(r_rays['ray_depth'][lo:hi]).any() and np.isnan(r_rays['ray_depth'][:lo]).all()
    SV.check_margins(r_rays, 'greedy')
    after_rays = SV.in_calls(SV.associate, rays, 1)[4]
    bridge = SV.in_calls(SV.associate, skip, 1)[4][lo - 1][0, 0]            # the root of slot 0 when it was last seen
    worst = 0.0
    for g in range(4, 30):                                                  # (g + 1) / 30 s after it: within max_age_s
        step = lo + g
        e_rays = SV.across(after_rays[step][0, 0, :3] - truth[step, 0], truth[step, 0], SV.STREAM_CAMERA)
        coasting = bridge[:3] + (step / SV.STREAM_FPS - bridge[27]) * bridge[3:6]
        e_skip = SV.across(coasting - truth[step, 0], truth[step, 0], SV.STREAM_CAMERA)
        assert e_rays < e_skip, (g, e_rays, e_skip)
        worst = max(worst, e_rays / e_skip)
    back = r_rays['cost'][hi]
    print(f"worst ratio of the errors across the ray, rays / skip: {worst:.3f}; cost at the return {back:.1f} mm "
          f"(the depth drifted: max_cost_mm is {rays['max_cost']:.0f})")
    assert back < rays['max_cost']


@pytest.mark.parametrize('steps_per_call', [1, 3, 8])
def test_stream_cut_into_calls_gives_the_ids_and_states_of_one_walk(host, steps_per_call):
    c = SV.stream_case('rays')
    for run in (SV.associate, host[2]):
        whole_id, whole_state, n_new, n_unplaced, _ = SV.in_calls(run, c, SV.STREAM_STEPS)
        got_id, got_state, got_new, got_unplaced, _ = SV.in_calls(run, c, steps_per_call)
        assert np.array_equal(got_id, whole_id) and (got_new, got_unplaced) == (n_new, n_unplaced) == (1, 0)
        assert set(got_state) == set(whole_state) == {0}
        for i, s in got_state.items():
            assert np.array_equal(s, whole_state[i], equal_nan=True), f'the state of id {i}, bit for bit'


# ---- the surface -----------------------------------------------------------------------------------------------------------------

NEW_SYMBOLS = (('metro_person_steps_labels', 13), ('metro_person_rays', 12), ('metro_associate_tracks_rays', 38))


def test_new_symbols_in_header_bindings_and_library(lib):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'metro_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(metro_[a-z0-9_]+)\s*\(', text))
    for name, n_args in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
        params = re.search(r'\b' + name + r'\s*\(([^)]*)\)', text).group(1)
        assert len(_lib.SIGNATURES[name][1]) == params.count(',') + 1 == n_args
    assert lib.metro_abi_version() == _lib.ABI_VERSION == 8                # the ABI is additive
    from metro_pose3d_amd import build
    assert 'person_rays.hip' in build.SOURCES
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert all(name in readme for name, _ in NEW_SYMBOLS) and 'follow_rig_poses_in_frames' in readme


def test_c_entries_reject_bad_arguments(lib):
    """Every return below comes before any launch: no device is needed."""
    cs = SPEC.to_c(_lib.METRO_PREC_F16)
    p = C.c_void_p(256)
    stp = [p, p, 4, p, 4, p, 2, p, p, p, p, p, None]
    assert lib.metro_person_steps_labels(*stp[:2], 129, *stp[3:]) == -1 and b'at most' in lib.metro_last_error()
    assert lib.metro_person_steps_labels(*stp[:2], -1, *stp[3:]) == -1 and b'negative' in lib.metro_last_error()
    for k in (0, 1, 3, 5, 7, 8, 9, 10, 11):
        a = list(stp)
        a[k] = None
        assert lib.metro_person_steps_labels(*a) == -1 and b'person_steps_labels' in lib.metro_last_error(), k
    assert lib.metro_person_steps_labels(*stp[:2], 0, *stp[3:]) == 0
    ray = [p, p, p, 8, C.byref(cs), p, _lib.METRO_TRI_COVARIANCE, p, 4, 2, p, None]
    assert lib.metro_person_rays(*ray[:6], 7, *ray[7:]) == -1 and b'weights' in lib.metro_last_error()
    assert lib.metro_person_rays(*ray[:3], 9, *ray[4:]) == -1 and b'crop rows' in lib.metro_last_error()
    assert lib.metro_person_rays(*ray[:8], 129, *ray[9:]) == -1 and b'at most' in lib.metro_last_error()
    assert lib.metro_person_rays(*ray[:4], None, *ray[5:]) == -1 and b'spec' in lib.metro_last_error()
    for k in (0, 1, 2, 5, 7, 10):
        a = list(ray)
        a[k] = None
        assert lib.metro_person_rays(*a) == -1 and b'person_rays' in lib.metro_last_error(), k
    assert lib.metro_person_rays(*ray[:3], 0, *ray[4:8], 0, *ray[9:]) == 0
    cs1 = _lib.MetroSpec(n_joints_out=17)
    cov = _lib.METRO_SMOOTH_COVARIANCE
    walk = [p, p, p, 4, p, 4, p, 2, C.byref(cs1), cov, 4e6, 1.0, 1.0, 2000.0, 0.0, 300.0, 600.0, 9, 1.0, p, 8] + [p] * 10 + \
           [0, p, p, 1000.0, p, p, None]
    assert len(walk) == 38

    def refused(k, v, word):
        a = list(walk)
        a[k] = v
        return lib.metro_associate_tracks_rays(*a) == -1 and word in lib.metro_last_error()
    assert refused(9, _lib.METRO_SMOOTH_ISOTROPIC, b'METRO_SMOOTH_COVARIANCE')
    assert refused(9, 5, b'measurement')
    assert refused(31, 2, b'assignment')
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        assert refused(34, bad, b'depth_sigma_mm'), bad
    assert refused(20, 129, b'track slots') and refused(10, 0.0, b'q must') and refused(17, 18, b'min_joints')
    for k in (0, 1, 2, 4, 6, 19, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 32, 33, 35, 36):
        assert refused(k, None, b'NULL'), k
    a = list(walk)
    a[3] = 0
    assert lib.metro_associate_tracks_rays(*a) == 0                        # no rows: nothing to launch


def test_python_surface_and_the_checks_before_the_library_is_touched(monkeypatch):
    import metro_pose3d_amd
    assert metro_pose3d_amd.follow_rig_poses_in_frames is FR.follow_rig_poses_in_frames
    assert 'follow_rig_poses_in_frames' in metro_pose3d_amd.__all__
    world = inspect.signature(FR.follow_world_poses_in_frames).parameters
    rig = inspect.signature(FR.follow_rig_poses_in_frames).parameters
    assert list(world)[:8] == ['frames', 'boxes', 'model_path', 'cameras', 'frame_index', 'timestamps', 'tracks', 'capacity']
    assert list(world)[-1] == 'assignment' and len(world) == 32, "follow_world_poses_in_frames' signature is unchanged"
    assert list(rig) == list(world) + ['single_view', 'ray_depth_sigma_mm']
    assert all(rig[k].default == world[k].default for k in world)
    assert rig['single_view'].default == 'rays' and rig['ray_depth_sigma_mm'].default == 1000.0
    assert FR.FollowedWorldPoses._fields == ('person_index', 'cost', 'n_pairs', 'world', 'world_covariance', 'person_step', 'track_index',
                                            'track_id', 'track_cost', 'n_new', 'n_dropped', 'tracks', 'smoothed')
    assert FR.FollowedRigPoses._fields == FR.FollowedWorldPoses._fields + ('single_view', 'ray_depth', 'n_unplaced')
    assert list(inspect.signature(MH.person_steps).parameters) == ['rows', 'starts', 'n_persons', 'box_step', 'step_times', 'n_views']
    assert list(inspect.signature(MH.associate_tracks).parameters)[-1] == 'assignment' and len(inspect.signature(MH.associate_tracks).parameters) == 19
    assert list(inspect.signature(MH.person_steps_labels).parameters) == ['person_index', 'n_persons', 'box_step', 'step_times']
    assert MH.RayAssociatedTracks._fields[:8] == MH.AssociatedTracks._fields
    init = list(inspect.signature(FR.Follower.__init__).parameters)
    assert init[:7] == ['self', 'model_path', 'cameras', 'world', 'assignment', 'capacity', 'single_view']
    # every refusal below comes before the library is loaded
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('the library was touched'))
    call = lambda **kw: FR.follow_rig_poses_in_frames(None, np.zeros((0, 4)), 'no-such-model', [], [], [], **kw)
    for kw, word in ((dict(single_view='both'), 'single_view'), (dict(single_view=None), 'single_view'),
                     (dict(ray_depth_sigma_mm=0.0), 'ray_depth_sigma_mm'), (dict(ray_depth_sigma_mm=float('nan')), 'ray_depth_sigma_mm'),
                     (dict(ray_depth_sigma_mm=float('inf')), 'ray_depth_sigma_mm'), (dict(ray_depth_sigma_mm='1000'), 'ray_depth_sigma_mm'),
                     (dict(single_view='skip', ray_depth_sigma_mm=-1.0), 'ray_depth_sigma_mm'),
                     (dict(measurement='isotropic'), 'isotropic'), (dict(assignment='best'), 'assignment')):
        with pytest.raises(ValueError, match=word):
            call(**kw)
    with pytest.raises(ValueError, match='world=True'):
        FR.Follower('m', [], single_view='rays')
    with pytest.raises(ValueError, match='single_view'):
        FR.Follower('m', [], world=True, single_view='both')
    with pytest.raises(ValueError, match='covariance'):
        FR.Follower('m', [], world=True, single_view='rays', measurement='isotropic')
    with pytest.raises(ValueError, match='ray_depth_sigma_mm'):
        FR.Follower('m', [], world=True, single_view='rays', ray_depth_sigma_mm=0)
    with pytest.raises(TypeError, match='ray_depth_sigma_mm'):
        FR.Follower('m', [], world=True, ray_depth_sigma_mm=500.0)             # without single_view it is what it was
    f = FR.Follower('m', [], world=True, single_view='rays', ray_depth_sigma_mm=500.0)
    assert f.single_view == 'rays' and f.keywords['ray_depth_sigma_mm'] == 500.0 and 'single_view' not in f.keywords
    assert FR.Follower('m', [], world=True).single_view is None and 'ray_depth_sigma_mm' not in FR.Follower('m', [], world=True).keywords
