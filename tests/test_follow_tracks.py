"""Boxes assigned to tracks over video, without a GPU: the fp64 restatement the GPU tests compare against
(tests/follow_tracks_ref.py) on known answers, a stream cut into calls, the kernel's own walk compiled for the host against
that restatement on every case, the margin that keeps every case away from a decision a last bit could flip, the argument
checks of the Python surface that run before any device is touched, and the new C symbols in header, bindings and library with
their invalid-argument returns."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from metro_pose3d_amd import _lib, frames as FR, heads as MH
from tests import follow_tracks_ref as FT
from tests.assoc_host import compile_walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = FT.CASES


def _ids_of(c, r, person):
    """The track ids of a person's boxes in time order."""
    rows = np.flatnonzero(c['person'] == person)
    return [int(r['track_id'][i]) for i in rows[np.argsort(c['times'][rows])]]


# ---- the restatement on known answers ------------------------------------------------------------------------------------------

def test_crossing_persons_keep_their_ids_where_the_nearest_rule_swaps_them():
    c, r = FT.case_and_expected('crossing')
    assert _ids_of(c, r, 0) == [0] * 9 and _ids_of(c, r, 1) == [1] * 9 and r['n_new'] == 2 and r['n_dropped'] == 0
    at4 = [c['poses'][i].astype(np.float64).mean(axis=0) for i in np.flatnonzero(c['times'] == 4 / 32.0)]
    assert np.abs(at4[0] - at4[1]).max() < 15.0, 'the two persons coincide at frame 4 (up to their build and the noise)'
    # a nearest-to-last-position rule (every track, in slot order, takes the unclaimed box whose centre is nearest to the centre
    # of its previous box) follows person 0 up to the crossing and then hands its track to person 1
    centre = lambda i: c['poses'][i].astype(np.float64).mean(axis=0)
    by_frame = [np.flatnonzero(c['times'] == f / 32.0) for f in range(9)]
    last = {int(c['person'][i]): centre(i) for i in by_frame[0]}
    followed = {0: [0], 1: [1]}
    for boxes in by_frame[1:]:
        left = list(boxes)
        for track in (0, 1):
            i = min(left, key=lambda i: np.linalg.norm(centre(i) - last[track]))
            left.remove(i)
            last[track] = centre(i)
            followed[track].append(int(c['person'][i]))
    assert followed[0][:5] == [0] * 5 and followed[0][5:] == [1] * 4 and followed[1][5:] == [0] * 4, followed


def test_absent_person_returns_under_its_id_within_max_age_and_under_a_new_one_beyond():
    c, r = FT.case_and_expected('absence-within')
    assert len(set(_ids_of(c, r, 0))) == 1 and len(_ids_of(c, r, 0)) == 8 and r['n_new'] == 2
    c, r = FT.case_and_expected('absence-beyond')
    ids = _ids_of(c, r, 0)
    assert ids[:4] == [ids[0]] * 4 and ids[4:] == [2] * 4 and ids[0] in (0, 1) and r['n_new'] == 3
    slots = r['track_index'][np.flatnonzero(c['person'] == 0)]
    assert len(set(slots.tolist())) == 2, 'no slot is retired inside a call: the person comes back in another slot'


def test_newcomer_gets_a_fresh_id():
    c, r = FT.case_and_expected('newcomer')
    assert _ids_of(c, r, 0) == [0] * 8 and _ids_of(c, r, 1) == [1] * 5 and r['n_new'] == 2
    born = np.flatnonzero(np.isnan(r['cost']) & (r['track_id'] >= 0))
    assert sorted(c['times'][born].tolist()) == [0.0, 3 / 32.0]


def test_of_two_boxes_near_one_track_the_nearer_continues_it():
    c, r = FT.case_and_expected('two-near-one')
    assert _ids_of(c, r, 0) == [0] * 6 and _ids_of(c, r, 1) == [1] * 3
    first_other = np.flatnonzero((c['person'] == 1) & (c['times'] == 3 / 32.0))[0]
    assert np.isnan(r['cost'][first_other]), 'the farther box is born although its cost was below max_cost_mm'
    assert r['margin_gate'] < 200, 'some cost of the case lies inside the gate: the farther box was a candidate'


def test_exact_ties_go_to_the_lowest_slot_then_the_lowest_position():
    c, r = FT.case_and_expected('ties')
    assert all(float(np.float32(v)) == v for v in c['poses'].reshape(-1))
    assert r['track_index'].tolist() == [0, 1, 2, 3] and r['track_id'].tolist() == [0, 1, 2, 3]
    assert r['cost'][:3].tolist() == [64.0, 64.0, 32.0] and np.isnan(r['cost'][3]) and r['n_new'] == 1


def test_exhausted_slots_leave_boxes_untracked_and_counted():
    c, r = FT.case_and_expected('exhausted')
    assert _ids_of(c, r, 0) == [0] * 4 and _ids_of(c, r, 1) == [1] * 4 and _ids_of(c, r, 2) == [-1] * 4
    assert (r['track_index'][c['person'] == 2] == -1).all() and r['n_dropped'] == 4 and r['n_new'] == 2 and r['next_id'] == 2


def test_box_without_a_finite_joint_is_untracked():
    c, r = FT.case_and_expected('nan-box')
    ids0, ids1 = _ids_of(c, r, 0), _ids_of(c, r, 1)
    assert ids0 == [0, 0, -1, 0, 0] or ids0 == [1, 1, -1, 1, 1]
    assert r['n_dropped'] == 1 and ids1[:3] == [ids1[0]] * 3 and ids1[3] == 2, 'too few joints to continue: born'
    assert r['n_new'] == 3


def test_slot_retired_at_call_start_is_reused_under_a_fresh_id():
    c, r = FT.case_and_expected('retired')
    assert _ids_of(c, r, 0) == [9] * 4 and _ids_of(c, r, 1) == [7] * 4 and r['ids'].tolist() == [9, 7, -1] and r['next_id'] == 10
    assert (r['track_index'][c['person'] == 0] == 0).all(), 'the retired slot is the lowest free one'
    assert np.isnan(r['state'][0, :, 27]).all() and (r['state'][1, :, 27] == -1 / 32.0).all()
    assert np.array_equal(r['state'][..., :27], c['state'][..., :27]), 'the retirement writes t_last only'


@pytest.mark.parametrize('name', list(CASES))
def test_margin_keeps_every_case_away_from_a_flip(name):
    """Every pick at least 1e-2 mm from every other finite cost of its row and column, every finite cost at least 1e-2 mm from
    max_cost_mm: a last-bit difference in a cost (the comparison allows 1e-3 mm) cannot change a decision."""
    c, r = FT.case_and_expected(name)
    print(f"{name}: pick margin {r['margin_pick']:.3g} mm, gate margin {r['margin_gate']:.3g} mm")
    assert r['margin_gate'] >= FT.MARGIN_MM
    assert c['tie'] or r['margin_pick'] >= FT.MARGIN_MM
    assert not c['tie'] or r['margin_pick'] == 0.0, 'the tie case does hold exact ties'


# ---- a stream cut into calls ----------------------------------------------------------------------------------------------------

def _stream():
    """70 frames: person 0 throughout, person 1 absent for frames 20-29 (within max_age_s), person 2 arriving at frame 33,
    person 3 leaving after frame 10 and back from frame 60 (beyond max_age_s: a new id)."""
    frames3 = list(range(11)) + list(range(60, 70))
    return FT.scene({0: FT._line((0, 0, 3000), (4, 1, 0), range(70)),
                     1: FT._line((1500, 0, 3200), (-3, 0, 2), [f for f in range(70) if not 20 <= f < 30]),
                     2: FT._line((-1500, 500, 3500), (2, -2, 0), range(33, 70)),
                     3: FT._line((3000, 0, 2800), (0, 1, 0), frames3)}, capacity=16, seed=31)


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
        # the smoothing launch that follows writes the working state into the table
        state, ids, next_id = r['working'], r['ids'], np.asarray([r['next_id']], np.int32).reshape(1)
    return track_id, {int(i): state[slot] for slot, i in enumerate(ids) if i >= 0}


@pytest.fixture(scope='module')
def stream_whole():
    c = _stream()
    return c, _in_calls(FT.associate, c, 70)


@pytest.mark.parametrize('frames_per_call', [1, 7, 64])
def test_stream_cut_into_calls_gives_the_ids_and_states_of_one_call(stream_whole, frames_per_call):
    c, (want_id, want_state) = stream_whole
    ids3 = want_id[c['person'] == 3][np.argsort(c['times'][c['person'] == 3])].tolist()
    assert ids3[:11] == [ids3[0]] * 11 and ids3[11:] == [4] * 10 and ids3[0] < 3, 'back after more than max_age_s: the fifth id'
    assert len(set(want_id[c['person'] == 1].tolist())) == 1 and set(want_id[c['person'] == 2].tolist()) == {3}
    got_id, got_state = _in_calls(FT.associate, c, frames_per_call)
    assert np.array_equal(got_id, want_id)
    assert len(got_state) >= 4 and set(got_state) <= set(want_state)
    for i, s in got_state.items():
        assert np.array_equal(s, want_state[i], equal_nan=True), f'the state of id {i}, bit for bit'


# ---- the kernel's own steps on the host ------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def host_kernel(tmp_path_factory):
    """associate_tracks.hip's walk, the function its kernels run, compiled for the host and run by one thread under the greedy
    rule without ray rows (tests/assoc_host.py); the dict it returns carries `smoothed_state`, what the smoothing kernel's code
    leaves in the table's state on the CSR the walk wrote."""
    return compile_walk(tmp_path_factory.mktemp('host_follow_tracks'), 'host_follow_tracks')[1]


@pytest.mark.parametrize('name', list(CASES))
def test_kernel_steps_on_the_host_match_the_restatement(host_kernel, name):
    """track_index, track_id, the CSR, the counts, the table's ids and next_id, the retired state, every t_last and the NaN
    patterns exactly; costs within 1e-3 mm.  x and P of the working state within 1e-9 of the slot's largest entry: the
    restatement inverts with LAPACK where the kernel uses cofactors, so their bits differ (the bound of
    tests/test_track_smoothing.py for the same pair); bit equality is asserted where both sides are the kernel's arithmetic --
    the working state against the smoothing kernel's own code run on the CSR the walk wrote."""
    c, want = FT.case_and_expected(name)
    got = host_kernel(c)
    worst = FT.compare(got, want, c)
    print(f'{name}: worst cost {worst[0]:.2e} mm, worst state {worst[1]:.2e} rel vs the fp64 restatement')
    assert not (got['track_index'] == FT.SENTINEL).any() and not (got['cost'] == FT.SENTINEL).any()
    assert np.array_equal(got['working'], got['smoothed_state'], equal_nan=True), 'the smoothing code leaves the working state, bit for bit'


@pytest.mark.parametrize('frames_per_call', [1, 7, 64])
def test_kernel_steps_on_the_host_cut_into_calls(host_kernel, stream_whole, frames_per_call):
    """The stream through the kernel's own steps, cut into calls: the restatement's ids, and per id the bits of one call."""
    c, (want_id, _) = stream_whole
    whole_id, whole_state = _in_calls(host_kernel, c, 70)
    got_id, got_state = _in_calls(host_kernel, c, frames_per_call)
    assert np.array_equal(whole_id, want_id) and np.array_equal(got_id, want_id)
    assert len(got_state) >= 4 and set(got_state) <= set(whole_state)
    for i, s in got_state.items():
        assert np.array_equal(s, whole_state[i], equal_nan=True), f'the state of id {i}, bit for bit'


# ---- the Python surface ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('ts', [[0.0, 0.0, 0.1, 0.1], [0.3, 0.1, 0.2, 0.1, 0.3, 0.0], [5.0], []],
                         ids=['ordered', 'unsorted', 'one', 'empty'])
def test_time_steps(ts):
    rows, starts = FR.time_steps(ts)
    assert rows.dtype == np.int32 and starts.dtype == np.int32 and starts[0] == 0 and starts[-1] == len(ts) == len(rows)
    want = [[i for i, t in enumerate(ts) if t == u] for u in sorted(set(ts))]
    assert [list(rows[starts[s]:starts[s + 1]]) for s in range(len(starts) - 1)] == want
    if len(ts):
        assert np.array_equal(FT.time_steps(ts)[0], rows) and np.array_equal(FT.time_steps(ts)[1], starts)


def test_new_track_table():
    t = FR.new_track_table(5, 17, 'cpu')
    assert isinstance(t, FR.TrackTable) and t._fields == ('state', 'ids', 'next_id')
    assert t.state.shape == (5, 17, 28) and t.state.dtype == torch.float64 and torch.isnan(t.state[..., 27]).all()
    assert t.ids.dtype == torch.int32 and t.ids.tolist() == [-1] * 5 and t.next_id.dtype == torch.int32 and t.next_id.tolist() == [0]
    for bad in (0, 129, -1, 2.0, True, None):
        with pytest.raises(ValueError, match='capacity'):
            FR.new_track_table(bad, 17, 'cpu')


def test_python_surface_checks_arguments_without_a_gpu():
    sig = inspect.signature(FR.follow_poses_in_frames)
    track = inspect.signature(FR.track_poses_in_frames).parameters
    rest = [p for p in track if p not in ('frames', 'boxes', 'model_path', 'cameras', 'track_index', 'frame_index', 'timestamps', 'state')]
    assert list(sig.parameters) == ['frames', 'boxes', 'model_path', 'cameras', 'frame_index', 'timestamps', 'tracks', 'capacity',
                                    'max_cost_mm', 'clip_mm', 'min_joints', 'max_age_s'] + rest
    for name in rest:
        assert sig.parameters[name].default == track[name].default
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d['tracks'], d['capacity'], d['max_cost_mm'], d['clip_mm'], d['min_joints'], d['max_age_s']) == (None, 64, 300.0, 600.0, None, 1.0)
    h = {k: v.default for k, v in inspect.signature(MH.associate_tracks).parameters.items()}
    for k in ('max_cost_mm', 'clip_mm', 'min_joints', 'max_age_s', 'measurement', 'accel_psd', 'sigma_floor_mm', 'cov_scale',
              'initial_speed_mm_s', 'gate'):
        assert h[k] == d[k]
    assert FR.FollowedPoses._fields == ('track_index', 'track_id', 'cost', 'n_new', 'n_dropped', 'tracks', 'smoothed')
    for word in ('design choices, not measurements', 'max_cost_mm', 'clip_mm', 'max_age_s', 'min_joints'):
        assert word in FR.follow_poses_in_frames.__doc__ and word in MH.associate_tracks.__doc__
    import metro_pose3d_amd
    assert metro_pose3d_amd.follow_poses_in_frames is FR.follow_poses_in_frames and 'follow_poses_in_frames' in metro_pose3d_amd.__all__
    frames = [np.zeros((8, 8, 3), np.uint8)] * 2
    boxes = [[0, 0, 4, 4], [1, 1, 4, 4]]
    from metro_pose3d_amd.camera import Camera
    cam = Camera(np.array([[500., 0, 4], [0, 500, 4], [0, 0, 1]]))
    call = lambda b=boxes, fi=(0, 1), ts=(0.0, 0.1), **kw: FR.follow_poses_in_frames(
        frames, b, 'no-such-model.npz', cam, fi, ts, **{'scale_recovery': 'true-root-depth', 'root_depth': [3000.0] * len(b), **kw})
    with pytest.raises(ValueError, match='root-relative'):
        call(scale_recovery='metro', root_depth=None)
    with pytest.raises(ValueError, match='at most 128'):
        call(b=[[0, 0, 4, 4]] * 129, fi=[0] * 129, ts=(0.0, 0.1))
    for bad in (0, 129, 64.0, None):
        with pytest.raises(ValueError, match='capacity'):
            call(capacity=bad)
    for key in ('max_cost_mm', 'clip_mm'):
        for bad in (0, -1.0, float('nan'), float('inf'), '1', True):
            with pytest.raises(ValueError, match=key):
                call(**{key: bad})
    for bad in (0, -1, 2.5, True, '3'):
        with pytest.raises(ValueError, match='min_joints'):
            call(min_joints=bad)
    for bad in (-0.1, float('nan'), '1', True, None):
        with pytest.raises(ValueError, match='max_age_s'):
            call(max_age_s=bad)
    with pytest.raises(ValueError, match='mode must be'):
        call(mode='rts')
    with pytest.raises(ValueError, match='accel_psd'):
        call(accel_psd=0)
    with pytest.raises(ValueError, match='one value per box'):
        call(fi=(0,))
    with pytest.raises(ValueError, match='finite'):
        call(ts=(0.0, float('nan')))
    good = FR.new_track_table(4, 17, 'cpu')
    for bad in ((good.state, good.ids), (good.state.float(), good.ids, good.next_id), (good.state, good.ids[:3], good.next_id),
                (good.state, good.ids.long(), good.next_id), good.state, (good.state[:, :, :27], good.ids, good.next_id)):
        with pytest.raises(ValueError, match='tracks must be'):
            call(tracks=bad)
    # heads.associate_tracks: checked before the library or a device is touched
    n, nj = 4, 17
    poses, cov = torch.zeros((n, nj, 3)), torch.zeros((n, nj, 3, 3))
    run = lambda p=poses, c=cov, t=(0.0, 0.0, 0.1, 0.1), rows=(0, 1, 2, 3), starts=(0, 2, 4), table=good, **kw: MH.associate_tracks(
        p, c, t, rows, starts, *table, **kw)
    with pytest.raises(ValueError, match='measurement must be'):
        run(measurement='diag')
    with pytest.raises(ValueError, match='max_cost_mm'):
        run(max_cost_mm=0)
    with pytest.raises(ValueError, match='max_age_s'):
        run(max_age_s=-1)
    with pytest.raises(ValueError, match='min_joints'):
        run(min_joints=18)
    with pytest.raises(ValueError, match='poses must be'):
        run(p=poses[..., :2])
    with pytest.raises(ValueError, match='needs covariance'):
        run(c=None)
    with pytest.raises(ValueError, match='one value per pose row'):
        run(t=(0.0, 0.1))
    with pytest.raises(ValueError, match='step_starts'):
        run(starts=())
    with pytest.raises(ValueError, match='at most 128'):
        run(p=torch.zeros((130, nj, 3)), c=None, measurement='isotropic', t=[0.0] * 130, rows=list(range(130)), starts=(0, 130))
    with pytest.raises(ValueError, match='state must be'):
        run(table=(torch.zeros((4, nj, 28)), good.ids, good.next_id))
    with pytest.raises(ValueError, match='state must be'):
        run(table=(torch.zeros((129, nj, 28), dtype=torch.float64), torch.zeros(129, dtype=torch.int32), good.next_id))
    with pytest.raises(ValueError, match='ids must be'):
        run(table=(good.state, good.ids[:3], good.next_id))
    with pytest.raises(ValueError, match='next_id must be'):
        run(table=(good.state, good.ids, good.next_id.long()))


def test_new_symbols_in_header_bindings_and_library(lib):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'metro_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(metro_[a-z0-9_]+)\s*\(', text))
    for name, n_args in (('metro_associate_tracks', 32), ('metro_associate_tracks_workspace_bytes', 2)):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
        params = re.search(r'\b' + name + r'\s*\(([^)]*)\)', text).group(1)
        assert len(_lib.SIGNATURES[name][1]) == params.count(',') + 1 == n_args
    assert re.search(r'#define\s+METRO_ASSOC_MAX\s+128\b', text) and _lib.METRO_ASSOC_MAX == MH.ASSOC_MAX == 128
    assert lib.metro_abi_version() == 8                    # the ABI is additive
    assert lib.metro_associate_tracks_workspace_bytes(64, 17) == 64 * 17 * 28 * 8
    assert lib.metro_associate_tracks_workspace_bytes(0, 17) == 0 and lib.metro_associate_tracks_workspace_bytes(-1, 17) == 0
    from metro_pose3d_amd import build
    assert 'associate_tracks.hip' in build.SOURCES and 'smooth_step.h' in build.HEADERS


def test_c_entry_rejects_bad_arguments(lib):
    """Every return below comes before any launch: no device is needed."""
    cs = _lib.MetroSpec(n_joints_out=17)
    p = C.c_void_p(256)
    fn = lib.metro_associate_tracks
    good = [p, p, p, 8, p, 8, p, 2, C.byref(cs), _lib.METRO_SMOOTH_COVARIANCE, 4e6, 1.0, 1.0, 2000.0, 0.0, 300.0, 600.0, 9, 1.0,
            p, 4, p, p, p, p, p, p, p, p, p, p, None]

    def call(**changes):
        a = list(good)
        for k, v in changes.items():
            a[int(k[1:])] = v
        return fn(*a)
    assert call(a8=None) == -1 and b'NULL spec' in lib.metro_last_error()
    for nj in (0, 65):
        assert call(a8=C.byref(_lib.MetroSpec(n_joints_out=nj))) == -1 and b'n_joints_out' in lib.metro_last_error()
    for bad in (-1, 2):
        assert call(a9=bad) == -1 and b'measurement' in lib.metro_last_error()
    for k in (3, 5, 7):                                     # n, n_step_rows, n_steps
        assert call(**{f'a{k}': -1}) == -1 and b'negative' in lib.metro_last_error()
    for bad in (0, -1, 129):
        assert call(a20=bad) == -1 and b'track slots' in lib.metro_last_error()
    nan = float('nan')
    for k, word in ((10, b'q must'), (11, b'r_floor'), (13, b'v0'), (15, b'max_cost_mm'), (16, b'clip_mm')):
        for bad in (0.0, -1.0, nan):
            assert call(**{f'a{k}': bad}) == -1 and word in lib.metro_last_error()
    for k, word in ((12, b'cov_scale'), (14, b'gate'), (18, b'max_age_s')):
        for bad in (-1.0, nan):
            assert call(**{f'a{k}': bad}) == -1 and word in lib.metro_last_error()
    for bad in (0, 18):
        assert call(a17=bad) == -1 and b'min_joints' in lib.metro_last_error()
    for k in (0, 2, 4, 6, 19, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30):
        assert call(**{f'a{k}': None}) == -1 and b'NULL poses' in lib.metro_last_error()
    assert call(a1=None) == -1 and b'covariance: NULL' in lib.metro_last_error()
    assert call(a1=None, a9=_lib.METRO_SMOOTH_ISOTROPIC, a3=0) == 0
    # nothing to do: no launch, whatever the pointers
    assert call(a3=0) == 0 and call(a5=0) == 0 and call(a7=0) == 0
    assert fn(*([None] * 3 + [0, None, 0, None, 0, C.byref(cs), 0, 4e6, 1.0, 0.0, 1.0, 0.0, 300.0, 600.0, 1, 0.0, None, 1] + [None] * 11)) == 0
