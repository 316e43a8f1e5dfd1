"""The association walk on the host: assoc_walk of associate_tracks.hip, the function the kernels run, compiled for the host and
executed by a team of ONE thread (its barrier does nothing, the least candidate is its own), the workgroup's LDS on the heap;
and smooth_tracks.hip's per-joint function for the state the smoothing launch leaves on the CSR and the arrays the walk wrote.
The wrapper builds its arguments with the builders the C entries use.  Shared by tests/test_follow_tracks.py (greedy),
tests/test_assign_tracks.py (optimal) and tests/test_single_view.py (ray rows, both rules)."""
import ctypes as C

import numpy as np

from metro_pose3d_amd import heads as MH
from tests import follow_tracks_ref as FT
from tests.helpers import compile_for_host

SOURCES = ['associate_tracks.hip', 'smooth_tracks.hip']
BODY = '''
#include <memory>
namespace {
// the visits of a search are the AssocCandD reductions since it started
struct AssocHostTeam {
    static constexpr int tid = 0, nt = 1;
    int visits = 0, most_visits = 0;
    void sync() const {}
    void search() { visits = 0; }
    metro::AssocCand least(metro::AssocCand own) const { return own; }
    metro::AssocCandD least(metro::AssocCandD own) {
        if (++visits > most_visits) most_visits = visits;
        return own;
    }
};
template <bool OPTIMAL, bool RAYS>
int host_walk(const metro::AssocRayArgs& a) {
    std::unique_ptr<metro::AssocLds> l(new metro::AssocLds);
    std::unique_ptr<metro::AssocOptLds> o(new metro::AssocOptLds);
    std::unique_ptr<metro::AssocRayLds> r(new metro::AssocRayLds);
    AssocHostTeam team;
    metro::assoc_walk<OPTIMAL, RAYS>(a, *l, *o, *r, team);
    return team.most_visits;
}
}
// ray rows iff single_box is given; without them the five arguments after `assignment` are not read
extern "C" void host_associate_tracks(float* poses, float* cov, const double* times, int n, const int* step_rows, int n_step_rows,
                                      const int* step_starts, int n_steps, int n_out, int measurement, double q, double r_floor,
                                      double cov_scale, double v0, double gate, float max_cost, double clip, int min_joints,
                                      double max_age, double* state, int n_tracks, int* ids, int* next_id, double* ws, int* track_index,
                                      int* track_id, float* cost_out, int* rows_out, int* starts_out, int* n_new, int* n_dropped,
                                      int assignment, const int* single_box, const double* rays, double depth_sigma, float* ray_depth,
                                      int* n_unplaced, int* most_visits) {
    const metro::AssocArgs base = metro::make_assoc_args(poses, cov, times, n, step_rows, n_step_rows, step_starts, n_steps, n_out,
                                                         measurement, q, r_floor, cov_scale, v0, gate, max_cost, clip, min_joints,
                                                         max_age, state, n_tracks, ids, next_id, ws, track_index, track_id, cost_out,
                                                         rows_out, starts_out, n_new, n_dropped);
    const metro::AssocRayArgs a = metro::make_assoc_ray_args(base, poses, cov, single_box, rays, depth_sigma, ray_depth, n_unplaced);
    most_visits[0] = single_box ? (assignment ? host_walk<true, true>(a) : host_walk<false, true>(a))
                                : (assignment ? host_walk<true, false>(a) : host_walk<false, false>(a));
}
extern "C" void host_filter_tracks(const float* poses, const float* cov, const double* times, int n, const int* rows, int n_rows,
                                   const int* starts, int n_tracks, int n_out, int measurement, double q, double r_floor,
                                   double cov_scale, double v0, double gate, double* state, float* poses_out, unsigned char* used) {
    const metro::SmoothArgs a = metro::make_smooth_args(poses, cov, times, n, rows, n_rows, starts, n_tracks, n_out, METRO_SMOOTH_FILTER,
                                                        measurement, q, r_floor, cov_scale, v0, gate, state, nullptr, poses_out, nullptr,
                                                        nullptr, used);
    for (int idx = 0; idx < n_tracks * n_out; ++idx) metro::smooth_track_joint(a, idx);
}
'''
P = C.c_void_p


def ptr(a):
    return P(a.ctypes.data if a is not None else 0)


def compile_walk(tmp, name, more_sources=(), more_body=''):
    """-> (the shared object of `more_sources` + SOURCES with `more_body` + BODY, associate)."""
    dll = compile_for_host(tmp, name, list(more_sources) + SOURCES, more_body + BODY)
    walk, flt = dll.host_associate_tracks, dll.host_filter_tracks
    walk.restype = flt.restype = None
    walk.argtypes = ([P, P, P, C.c_int, P, C.c_int, P, C.c_int, C.c_int, C.c_int] + [C.c_double] * 5 +
                     [C.c_float, C.c_double, C.c_int, C.c_double, P, C.c_int] + [P] * 10 + [C.c_int, P, P, C.c_double, P, P, P])
    flt.argtypes = [P, P, P, C.c_int, P, C.c_int, P, C.c_int, C.c_int, C.c_int] + [C.c_double] * 5 + [P, P, P]

    def associate(c, assignment='greedy', ray_rows=False):
        """The walk over case `c` under one rule, with c's single_box, rays and depth_sigma if `ray_rows` -> the dict the
        comparisons read, every output pre-filled with the sentinel: the walk's outputs, the table after it (state, ids,
        next_id), `working`, the `poses` and `cov` it read (with ray rows: and wrote), `ray_depth` and `n_unplaced` (the sentinel
        without ray rows), `smoothed_state` and `used` (what the smoothing kernel's code in filter mode leaves on the CSR and
        the arrays the walk wrote) and `most_visits` of any search of the optimal rule."""
        poses = np.array(c['poses'], np.float32)
        n, nj = poses.shape[:2]
        cov = None if c['cov'] is None else np.array(c['cov'], np.float32).reshape(n, nj, 9)
        times = np.ascontiguousarray(c['times'], np.float64)
        step_rows, step_starts = np.ascontiguousarray(c['step_rows'], np.int32), np.ascontiguousarray(c['step_starts'], np.int32)
        state, ids, next_id = np.array(c['state'], np.float64), np.array(c['ids'], np.int32), np.array(c['next_id'], np.int32).reshape(1)
        single, ray_in, depth_sigma = None, None, 0.0
        if ray_rows:
            single, ray_in = np.ascontiguousarray(c['single_box'], np.int32), np.ascontiguousarray(c['rays'], np.float64)
            depth_sigma = float(c['depth_sigma'])
        cap = len(ids)
        ws = np.full((cap, nj, 28), float(FT.SENTINEL))
        ints = lambda k: np.full(k, FT.SENTINEL, np.int32)
        track_index, track_id, rows, starts, n_new, n_dropped, n_unplaced, visits = (ints(k) for k in (n, n, n, cap + 1, 1, 1, 1, 1))
        cost, depth = np.full(n, float(FT.SENTINEL), np.float32), np.full((n, nj), float(FT.SENTINEL), np.float32)
        kind = MH.SMOOTH_MEASUREMENTS[c['measurement']]
        walk(ptr(poses), ptr(cov), ptr(times), n, ptr(step_rows), len(step_rows), ptr(step_starts), len(step_starts) - 1, nj, kind,
             c['q'], c['r_floor'], c['cov_scale'], c['v0'], c['gate'], c['max_cost'], c['clip'], c['min_joints'], c['max_age'], ptr(state),
             cap, ptr(ids), ptr(next_id), ptr(ws), ptr(track_index), ptr(track_id), ptr(cost), ptr(rows), ptr(starts), ptr(n_new),
             ptr(n_dropped), int(assignment == 'optimal'), ptr(single), ptr(ray_in), depth_sigma, ptr(depth), ptr(n_unplaced), ptr(visits))
        smoothed, poses_out, used = state.copy(), np.empty((n, nj, 3), np.float32), np.zeros((n, nj), np.uint8)
        flt(ptr(poses), ptr(cov), ptr(times), n, ptr(rows), n, ptr(starts), cap, nj, kind, c['q'], c['r_floor'], c['cov_scale'], c['v0'],
            c['gate'], ptr(smoothed), ptr(poses_out), ptr(used))
        return dict(track_index=track_index, track_id=track_id, cost=cost, rows=rows, starts=starts, n_new=n_new, n_dropped=n_dropped,
                    n_unplaced=n_unplaced, state=state, ids=ids, next_id=int(next_id[0]), working=ws, poses=poses, cov=cov,
                    ray_depth=depth, smoothed_state=smoothed, used=used, most_visits=int(visits[0]))
    return dll, associate


# ---- the walk with ray rows switched on but no ray row among the boxes is the walk without them ----------------------------------

# The cases of assign_tracks_ref.CASES whose measurement is 'covariance' (the ray entry takes no other), for either rule: they
# hold follow_tracks_ref's as 'followed-*'.  Among them T128-m128-j17 (128 slots against 128 boxes in one step: every wave in
# the reduction, the full cost matrix), chain (a search of three visits) and followed-retired (a slot retired at the start).
NO_RAY_ROW_CASES = ('trap', 'not-cardinality', 'chain', 'all-inadmissible', 'empty-table', 'full-table', 'stream', 'T1-m1', 'T1-m2',
                    'T2-m1', 'T2-m2-j64-steps2', 'T64-m63', 'T128-m128-j17') + tuple('followed-' + name for name in (
                        'crossing', 'absence-within', 'absence-beyond', 'newcomer', 'two-near-one', 'exhausted', 'nan-box', 'retired',
                        'skipped', 'cap1-box1-step1', 'cap1-box2', 'cap65-box64', 'cap65-box65-j1', 'cap128-box128-j1', 'j64', 'steps65'))
SHARED_OUTPUTS = ('track_index', 'track_id', 'cost', 'rows', 'starts', 'n_new', 'n_dropped', 'state', 'ids', 'next_id', 'working')


def without_ray_rows(c):
    """Case `c` as the ray entry takes it when no row is a ray row: single_box all -1 and rays nobody may read (NaN)."""
    assert c['measurement'] == 'covariance'
    n, nj = np.asarray(c['poses']).shape[:2]
    return dict(c, single_box=np.full(n, -1, np.int32), rays=np.full((n, nj, 8), np.nan), depth_sigma=1000.0)


def assert_ray_walk_is_the_plain_walk(rays, plain, c):
    """`rays`: the outputs of the ray walk over without_ray_rows(c) (ray_depth and n_unplaced pre-filled with the sentinel, poses
    and cov as it left them); `plain`: those of the walk without ray rows over c.  Every shared output bit for bit, nothing
    unplaced, poses and covariance untouched; ray_depth is NaN throughout, as for any row that is not placed."""
    for k in SHARED_OUTPUTS:
        assert np.array_equal(np.asarray(rays[k]), np.asarray(plain[k]), equal_nan=True), k
    assert int(np.asarray(rays['n_unplaced']).reshape(-1)[0]) == 0
    n, nj = np.asarray(c['poses']).shape[:2]
    assert np.array_equal(np.asarray(rays['poses']), np.asarray(c['poses'], np.float32), equal_nan=True), 'poses untouched'
    assert np.array_equal(np.asarray(rays['cov']).reshape(n, nj, 9), np.asarray(c['cov'], np.float32).reshape(n, nj, 9),
                          equal_nan=True), 'covariance untouched'
    assert np.isnan(np.asarray(rays['ray_depth'])).all()
