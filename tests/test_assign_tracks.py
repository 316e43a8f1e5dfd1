"""The optimal box-to-track assignment, without a GPU: the fp64 restatement (tests/assign_tracks_ref.py) on known answers and
against the greedy rule, its two solvers against each other (and scipy where it imports), the margins that keep every case away
from a decision a last bit could flip, a stream cut into calls, the kernel's own walk compiled for the host against the
restatement on every case, the new C symbol in header, bindings and library with its invalid-argument returns, the
`assignment` keyword and frames.Follower's construction."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from metro_pose3d_amd import _lib, frames as FR, heads as MH
from tests import assign_tracks_ref as AR
from tests import follow_tracks_ref as FT
from tests.assoc_host import compile_walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = AR.CASES


def _ids_of(c, r, person):
    rows = np.flatnonzero(c['person'] == person)
    return [int(r['track_id'][i]) for i in rows[np.argsort(c['times'][rows], kind='stable')]]


# ---- the restatement on known answers ------------------------------------------------------------------------------------------

def test_trap_scene_keeps_both_ids_where_greedy_swaps_them():
    c, r = AR.case_and_expected('trap')
    assert r['track_id'].tolist() == [0, 0, 0, 1, 1, 1] and r['n_new'] == 2 and r['n_dropped'] == 0
    assert abs(r['cost'][2] - 120.0) < 1e-3 and abs(r['cost'][5] - 130.0) < 1e-3
    assert abs(r['margin_opt'] - 150.0) < 1e-2, 'the second-best assignment is 150 mm away'
    greedy = FT.associate(c)
    assert greedy['track_id'].tolist() == [0, 0, 2, 1, 1, 0] and greedy['n_new'] == 3
    assert abs(greedy['cost'][5] - 100.0) < 1e-3 and np.isnan(greedy['cost'][2])


def test_one_near_pair_beats_two_far_ones():
    c, r = AR.case_and_expected('not-cardinality')
    assert r['track_index'].tolist() == [0, 2] and r['n_pairs'] == 1 and r['n_new'] == 1
    assert abs(r['cost'][0] - 10.0) < 1e-3 and np.isnan(r['cost'][1])
    t = 1 / 32.0
    costs = [[float(FT._cost(c['state'][s], c['poses'][b].astype(np.float64), t, c)) for b in (0, 1)] for s in (0, 1)]
    assert abs(costs[0][0] - 10) < 1e-3 and abs(costs[0][1] - 299) < 1e-3 and abs(costs[1][0] - 299) < 1e-3 and costs[1][1] == np.inf


def test_third_box_finds_its_slot_through_a_path_of_length_three():
    c, r = AR.case_and_expected('chain')
    assert r['track_index'].tolist() == [1, 2, 0] and r['n_new'] == 0
    assert np.abs(r['cost'] - [130.0, 130.0, 170.0]).max() < 1e-3
    greedy = FT.associate(c)
    assert greedy['track_index'].tolist()[:2] == [0, 1] and greedy['n_new'] == 1, 'greedy keeps the two nearest pairs and bears the third box'


def test_boxes_without_an_admissible_slot_are_born_and_a_full_table_drops_them():
    c, r = AR.case_and_expected('all-inadmissible')
    assert r['n_pairs'] == 0 and r['n_new'] == 3 and r['track_index'].tolist() == [2, 3, 4] and np.isnan(r['cost']).all()
    c, r = AR.case_and_expected('empty-table')
    assert r['n_new'] == 3 and _ids_of(c, r, 0) == [0, 0] and _ids_of(c, r, 1) == [1, 1] and _ids_of(c, r, 2) == [2]
    c, r = AR.case_and_expected('full-table')
    assert r['track_index'].tolist() == [0, 1, 2, -1, -1] and r['n_dropped'] == 2 and r['n_new'] == 0


def test_old_slot_nan_box_and_crossing_under_the_optimal_rule():
    c, r = AR.case_and_expected('followed-absence-beyond')
    ids = _ids_of(c, r, 0)
    assert ids[:4] == [ids[0]] * 4 and ids[4:] == [2] * 4 and r['n_new'] == 3, 'a slot older than max_age_s is a +inf row'
    c, r = AR.case_and_expected('followed-nan-box')
    assert r['n_dropped'] == 1 and r['n_new'] == 3
    c, r = AR.case_and_expected('followed-crossing')
    assert _ids_of(c, r, 0) == [0] * 9 and _ids_of(c, r, 1) == [1] * 9
    g = FT.case_and_expected('crossing')[1]
    assert np.array_equal(g['track_id'], r['track_id']), 'walking through each other: the same ids under both rules'
    c, r = AR.case_and_expected('followed-exhausted')
    assert r['n_dropped'] == 4 and r['n_new'] == 2


def test_line_of_persons_has_several_admissible_slots_per_box():
    c, r = AR.case_and_expected('T128-m128-j17')
    t = 1 / 32.0
    for b in range(128):
        row = [FT._cost(c['state'][s], c['poses'][b].astype(np.float64), t, c) for s in range(max(b - 3, 0), min(b + 4, 128))]
        assert sum(v < 300.0 for v in row) >= 3, b
    greedy = FT.associate(c)
    assert r['n_pairs'] >= 120 and not np.array_equal(greedy['track_index'], r['track_index'])
    gain = lambda x: float((300.0 - x['cost'][~np.isnan(x['cost'])].astype(np.float64)).sum())
    assert gain(r) > gain(greedy) + 100.0, 'the optimum gains more than greedy does'


def test_solvers_agree_with_each_other_and_with_scipy():
    rng = np.random.default_rng(5)
    try:
        from scipy.optimize import linear_sum_assignment
    except ImportError:
        linear_sum_assignment = None
    for trial in range(120):
        nk, ns = rng.integers(1, 7, 2) if trial < 100 else rng.integers(8, 20, 2)
        cost = rng.uniform(0, 500, (nk, ns))
        cost[rng.random((nk, ns)) < 0.2] = np.inf
        w = np.where(cost < 300.0, cost - 300.0, np.inf)
        total, pairs, margin = AR.solve(w)                 # asserts exhaustive == paths and both second-best totals where both apply
        assert len(set(pairs.values())) == len(pairs) and all(np.isfinite(w[b, s]) for b, s in pairs.items()) and margin >= 0
        if linear_sum_assignment is not None:
            padded = np.concatenate([np.minimum(cost, 300.0), np.full((nk, nk), 300.0)], axis=1)
            rows, cols = linear_sum_assignment(padded)
            assert abs((padded[rows, cols] - 300.0).sum() - total) < 1e-9


@pytest.mark.parametrize('name', list(CASES))
def test_margins_keep_every_case_away_from_a_flip(name):
    """Every finite cost at least 1e-2 mm from max_cost_mm, and the second-best assignment of every step at least
    max(1e-2, 2 min(T, m) 1e-3) mm above the optimum: the 1e-3 mm allowed per cost cannot change a decision."""
    c, r = AR.case_and_expected(name)
    print(f"{name}: gap to the second-best assignment {r['margin_opt']:.4g} mm (needed {r['margin_needed']:.3g}), "
          f"gate margin {r['margin_gate']:.3g} mm")
    assert r['margin_gate'] >= AR.MARGIN_MM
    if c['tie']:
        assert name != 'tie' or r['margin_opt'] == 0.0, 'the tie case does hold two equal optima'
    else:
        assert r['margin_opt'] >= r['margin_needed']


# ---- a stream cut into calls ----------------------------------------------------------------------------------------------------

def _in_calls(run, c, frames_per_call):
    """The stream in calls of `frames_per_call` steps, the table carried -> (track_id [n], {id: state of its slot})."""
    state, ids, next_id = FT.new_table(len(c['ids']), c['poses'].shape[1])
    starts, track_id = c['step_starts'], np.full(len(c['poses']), -1, np.int32)
    for s in range(0, len(starts) - 1, frames_per_call):
        e = min(s + frames_per_call, len(starts) - 1)
        part = dict(c, step_rows=c['step_rows'][starts[s]:starts[e]], step_starts=starts[s:e + 1] - starts[s], state=state, ids=ids,
                    next_id=next_id)
        r = run(part)
        listed = part['step_rows']
        track_id[listed] = r['track_id'][listed]
        state, ids, next_id = r['working'], r['ids'], np.asarray([r['next_id']], np.int32).reshape(1)
    return track_id, {int(i): state[slot] for slot, i in enumerate(ids) if i >= 0}


@pytest.fixture(scope='module')
def stream_whole():
    c = AR.case_and_expected('stream')[0]
    return c, _in_calls(AR.associate, c, 9)


@pytest.mark.parametrize('frames_per_call', [1, 3])
def test_stream_cut_into_calls_gives_the_ids_and_states_of_one_call(stream_whole, frames_per_call):
    c, (want_id, want_state) = stream_whole
    assert all(len(set(want_id[c['person'] == p].tolist())) == 1 for p in range(4)), 'every person keeps one id'
    got_id, got_state = _in_calls(AR.associate, c, frames_per_call)
    assert np.array_equal(got_id, want_id) and set(got_state) == set(want_state)
    for i, s in got_state.items():
        assert np.array_equal(s, want_state[i], equal_nan=True), f'the state of id {i}, bit for bit'


# ---- the kernel's own steps on the host ------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def host_kernel(tmp_path_factory):
    """associate_tracks.hip's walk, the function its kernels run, compiled for the host and run by one thread under the optimal
    rule without ray rows (tests/assoc_host.py); the dict it returns carries `smoothed_state` and `most_visits`, the visits of
    the longest search, which the one-thread team counts."""
    associate = compile_walk(tmp_path_factory.mktemp('host_assign_tracks'), 'host_assign_tracks')[1]
    return lambda c: associate(c, 'optimal')


@pytest.mark.parametrize('name', list(CASES))
def test_kernel_steps_on_the_host_match_the_restatement(host_kernel, name):
    """Slots, ids, the CSR, the counts, every t_last and the NaN patterns exactly; costs within 1e-3 mm; x and P of the working
    state within 1e-9 of the slot's largest entry (LAPACK there, cofactors here); bit for bit what the smoothing kernel's own
    code leaves on the CSR the walk wrote.  A case of exact ties is held to the properties every optimum shares, and two runs
    to identical outputs."""
    c, want = AR.case_and_expected(name)
    got = host_kernel(c)
    worst = AR.compare(got, want, c)
    print(f'{name}: worst cost {worst[0]:.2e} mm, worst state {worst[1]:.2e} rel vs the fp64 restatement; most visits of a search '
          f"{got['most_visits']}")
    assert not (got['track_index'] == FT.SENTINEL).any() and not (got['cost'] == FT.SENTINEL).any()
    assert np.array_equal(got['working'], got['smoothed_state'], equal_nan=True), 'the smoothing code leaves the working state, bit for bit'
    assert got['most_visits'] <= len(c['ids']) + 1
    if c['tie']:
        again = host_kernel(c)
        for k in ('track_index', 'track_id', 'cost', 'rows', 'starts', 'ids', 'working'):
            assert np.array_equal(got[k], again[k], equal_nan=True), k


def test_kernel_steps_take_a_real_path_in_the_chain_and_on_the_line(host_kernel):
    assert host_kernel(AR.case_and_expected('chain')[0])['most_visits'] == 3
    assert host_kernel(AR.case_and_expected('T128-m128-j17')[0])['most_visits'] >= 3


@pytest.mark.parametrize('frames_per_call', [1, 3])
def test_kernel_steps_on_the_host_cut_into_calls(host_kernel, stream_whole, frames_per_call):
    c, (want_id, _) = stream_whole
    whole_id, whole_state = _in_calls(host_kernel, c, 9)
    got_id, got_state = _in_calls(host_kernel, c, frames_per_call)
    assert np.array_equal(whole_id, want_id) and np.array_equal(got_id, want_id)
    assert set(got_state) == set(whole_state)
    for i, s in got_state.items():
        assert np.array_equal(s, whole_state[i], equal_nan=True), f'the state of id {i}, bit for bit'


# ---- the C symbol ---------------------------------------------------------------------------------------------------------------

def test_new_symbol_in_header_bindings_and_library(lib):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'metro_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(metro_[a-z0-9_]+)\s*\(', text))
    name = 'metro_associate_tracks_optimal'
    assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
    params = re.search(r'\b' + name + r'\s*\(([^)]*)\)', text).group(1)
    greedy = re.search(r'\bmetro_associate_tracks\s*\(([^)]*)\)', text).group(1)
    assert len(_lib.SIGNATURES[name][1]) == params.count(',') + 1 == 32
    assert re.sub(r'\s+', ' ', params) == re.sub(r'\s+', ' ', greedy), "metro_associate_tracks' parameter list"
    assert [a for a in _lib.SIGNATURES[name][1]] == [a for a in _lib.SIGNATURES['metro_associate_tracks'][1]]
    assert lib.metro_abi_version() == _lib.ABI_VERSION == 8       # the ABI is additive
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert name in integration and name in open(os.path.join(ROOT, 'README.md')).read()


def test_c_entry_rejects_what_the_greedy_entry_rejects(lib):
    """Every return below comes before any launch: no device is needed.  Both entries get the same arguments."""
    cs = _lib.MetroSpec(n_joints_out=17)
    p = C.c_void_p(256)
    good = [p, p, p, 8, p, 8, p, 2, C.byref(cs), _lib.METRO_SMOOTH_COVARIANCE, 4e6, 1.0, 1.0, 2000.0, 0.0, 300.0, 600.0, 9, 1.0,
            p, 4, p, p, p, p, p, p, p, p, p, p, None]
    nan = float('nan')
    bad = [({8: None}, b'NULL spec')]
    bad += [({8: C.byref(_lib.MetroSpec(n_joints_out=nj))}, b'n_joints_out') for nj in (0, 65)]
    bad += [({9: v}, b'measurement') for v in (-1, 2)]
    bad += [({k: -1}, b'negative') for k in (3, 5, 7)]
    bad += [({20: v}, b'track slots') for v in (0, -1, 129)]
    bad += [({k: v}, word) for k, word in ((10, b'q must'), (11, b'r_floor'), (13, b'v0'), (15, b'max_cost_mm'), (16, b'clip_mm'))
            for v in (0.0, -1.0, nan)]
    bad += [({k: v}, word) for k, word in ((12, b'cov_scale'), (14, b'gate'), (18, b'max_age_s')) for v in (-1.0, nan)]
    bad += [({17: v}, b'min_joints') for v in (0, 18)]
    bad += [({k: None}, b'NULL poses') for k in (0, 2, 4, 6, 19, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30)]
    bad += [({1: None}, b'covariance: NULL')]
    for changes, word in bad:
        a = list(good)
        for k, v in changes.items():
            a[k] = v
        assert lib.metro_associate_tracks(*a) == -1 and word in lib.metro_last_error(), (changes, 'greedy')
        assert lib.metro_associate_tracks_optimal(*a) == -1 and word in lib.metro_last_error(), changes
    fn = lib.metro_associate_tracks_optimal
    for k in (3, 5, 7):                                    # nothing to do: no launch, whatever the pointers
        a = list(good)
        a[k] = 0
        assert fn(*a) == 0
    assert fn(*([None] * 3 + [0, None, 0, None, 0, C.byref(cs), 0, 4e6, 1.0, 0.0, 1.0, 0.0, 300.0, 600.0, 1, 0.0, None, 1] + [None] * 11)) == 0


# ---- the Python surface ---------------------------------------------------------------------------------------------------------

def _associate(**kw):
    table = FR.new_track_table(4, 17, 'cpu')
    return MH.associate_tracks(torch.zeros((4, 17, 3)), torch.zeros((4, 17, 3, 3)), (0.0, 0.0, 0.1, 0.1), (0, 1, 2, 3), (0, 2, 4), *table, **kw)


def test_assignment_keyword_is_checked_before_the_library_is_touched(monkeypatch):
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('the library was touched'))
    sig = inspect.signature(MH.associate_tracks)
    assert list(sig.parameters)[-1] == 'assignment' and sig.parameters['assignment'].default == 'greedy'
    for bad in ('best', 'Optimal', '', None, 1, True, b'optimal'):
        with pytest.raises(ValueError, match='assignment'):
            _associate(assignment=bad)
    with pytest.raises(ValueError, match='max_cost_mm'):    # a good rule does not hide the other checks
        _associate(assignment='optimal', max_cost_mm=0)
    for word in ('admissible', 'total gain', "'optimal'", "'greedy'", 'not a maximum-cardinality', 'design choices, not measurements'):
        assert word in MH.associate_tracks.__doc__, word


def test_follow_calls_take_the_rule_where_their_signature_allows():
    world = inspect.signature(FR.follow_world_poses_in_frames).parameters
    assert list(world)[-2:] == ['crop_dtype', 'assignment'] and world['assignment'].default == 'greedy'
    assert 'assignment' not in inspect.signature(FR.follow_poses_in_frames).parameters, 'its parameter list is pinned'
    from metro_pose3d_amd.camera import Camera
    cam = Camera(np.array([[500., 0, 4], [0, 500, 4], [0, 0, 1]]))
    frames = [np.zeros((8, 8, 3), np.uint8)] * 2
    for bad in ('best', None, 2):
        with pytest.raises(ValueError, match='assignment'):
            FR.follow_world_poses_in_frames(frames, [[0, 0, 4, 4], [1, 1, 4, 4]], 'no-such-model.npz', [cam, cam], (0, 1), (0.0, 0.0),
                                            assignment=bad)
        with pytest.raises(ValueError, match='assignment'):     # the one road of a rule to one-camera following: the group, built
            MH.Association.checked(300.0, 600.0, None, 1.0, bad)  # by Follower
        with pytest.raises(ValueError, match='assignment'):
            FR.Follower('no-such-model.npz', cam, assignment=bad)


def test_follower_checks_its_keywords_at_construction():
    import metro_pose3d_amd
    assert metro_pose3d_amd.Follower is FR.Follower and 'Follower' in metro_pose3d_amd.__all__
    from metro_pose3d_amd.camera import Camera
    cam = Camera(np.array([[500., 0, 4], [0, 500, 4], [0, 0, 1]]))
    sig = inspect.signature(FR.Follower.__init__).parameters
    assert list(sig)[1:6] == ['model_path', 'cameras', 'world', 'assignment', 'capacity']
    assert (sig['world'].default, sig['assignment'].default, sig['capacity'].default) == (False, 'greedy', 64)
    f = FR.Follower('no-such-model.npz', cam)
    assert f.tracks is None and f.assignment == 'greedy' and not f.world and f.capacity == 64
    f.reset()
    assert f.tracks is None
    with pytest.raises(ValueError, match='follow first'):
        f.predict([[8, 8]], [0.0])
    follow = inspect.signature(FR.follow_poses_in_frames).parameters
    given = ('frames', 'boxes', 'model_path', 'cameras', 'frame_index', 'timestamps', 'tracks', 'capacity')
    assert f.keywords == {k: p.default for k, p in follow.items() if k not in given}
    w = FR.Follower('no-such-model.npz', [cam, cam], world=True, assignment='optimal', capacity=8, match_max_cost_mm=150.0)
    world = inspect.signature(FR.follow_world_poses_in_frames).parameters
    assert set(w.keywords) == set(world) - set(given) - {'assignment'} and w.keywords['match_max_cost_mm'] == 150.0 and w.world
    for bad in ('frames', 'tracks', 'timestamps', 'no_such_keyword', 'match_clip_mm', 'weights'):
        with pytest.raises(TypeError, match=bad):
            FR.Follower('no-such-model.npz', cam, **{bad: 1})
    for bad in ('scale_recovery', 'root_depth', 'coords', 'frame_index'):
        with pytest.raises(TypeError, match=bad):
            FR.Follower('no-such-model.npz', [cam, cam], world=True, **{bad: 'camera'})
    for world_flag in (False, True):
        make = lambda **kw: FR.Follower('no-such-model.npz', [cam, cam] if world_flag else cam, world=world_flag, **kw)
        with pytest.raises(ValueError, match='assignment'):
            make(assignment='best')
        for bad in (0, 129, 64.0, None):
            with pytest.raises(ValueError, match='capacity'):
                make(capacity=bad)
        for key, bad in (('max_cost_mm', 0), ('clip_mm', float('nan')), ('min_joints', 2.5), ('max_age_s', -0.1), ('accel_psd', 0),
                         ('measurement', 'diag')):
            with pytest.raises(ValueError, match=key):
                make(**{key: bad})
        with pytest.raises(ValueError, match='mode must be'):
            make(mode='rts')
    with pytest.raises(ValueError, match='match_max_cost_mm|max_cost_mm'):
        FR.Follower('no-such-model.npz', [cam, cam], world=True, match_max_cost_mm=-1.0)
    with pytest.raises(ValueError):
        FR.Follower('no-such-model.npz', [cam, cam], world=True, min_angle_deg=-1.0)
    with pytest.raises(ValueError, match='root-relative'):
        FR.Follower('no-such-model.npz', cam, scale_recovery='metro')
    with pytest.raises(ValueError, match='world'):
        FR.Follower('no-such-model.npz', cam, world='yes')
