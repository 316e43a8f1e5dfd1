"""Tracked poses smoothed over video, without a GPU: the fp64 restatement the GPU tests compare against
(tests/track_smoothing_ref.py) on known answers and on a synthetic noisy track, the kernel's own per-joint code compiled for
the host against that restatement, the carried state, the CSR grouping, the argument checks of the Python surface that run
before any device is touched, and the new C symbols in header, bindings and library with their invalid-argument returns."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from metro_pose3d_amd import _lib, frames as FR, heads as MH
from tests import track_smoothing_ref as TS
from tests.helpers import compile_for_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES, MODES, MEASUREMENTS = TS.CASES, TS.MODES, TS.MEASUREMENTS


# ---- the restatement on known answers ------------------------------------------------------------------------------------------

def _one_track(z, cov=None, fps=30.0):
    """T rows of one joint, one track in memory order."""
    n = len(z)
    return dict(poses=np.asarray(z, np.float32).reshape(n, 1, 3), cov=cov, times=np.arange(n) / fps, rows=np.arange(n, dtype=np.int32),
                starts=np.asarray([0, n], np.int32))


@pytest.mark.parametrize('q,sigma', [(4e6, 10.0), (4e6, 1.0), (1e4, 30.0)])
def test_steady_state_gain_is_the_alpha_beta_gain(q, sigma):
    """Isotropic noise, no gaps: after 400 steps the filter's position gain K_pp = P_pp / sigma^2 (the filtered position
    variance over the measurement's) is the closed-form alpha of the alpha-beta filter for this process noise
    (TS.alpha_beta_gain), within 1e-9."""
    c = _one_track(np.zeros((400, 3)))
    _, _, cov, _, _ = TS.smooth_tracks(c['poses'], None, c['times'], c['rows'], c['starts'], 'filter', 'isotropic', q=q, r_floor=sigma)
    gain = cov[-1, 0].reshape(3, 3) / sigma ** 2
    want = TS.alpha_beta_gain(q, 1 / 30.0, sigma)
    print(f'q {q:g}, sigma {sigma:g}: gain {gain[0, 0]:.12f}, closed form {want:.12f}')
    assert 0 < want < 1 and np.abs(gain - want * np.eye(3)).max() <= 1e-9


@pytest.mark.parametrize('mode', MODES)
def test_exact_constant_velocity_track_is_returned(mode):
    """Positions exactly on p0 + v t (values and times exact in fp32 / binary), measured with sigma = 1 mm and a first velocity
    left open (v0 = 1e8 mm/s): the second row fixes the velocity up to (2 R + q dt^3 / 3) / (v0 dt)^2 = 4e-12 of it, every
    later innovation is fp64 noise, so positions come back within 1e-6 mm and the velocity within 1e-3 mm/s (the filter from
    its second row, the smoother on every row)."""
    v, p0, t = np.array([1024.0, -512.0, 256.0]), np.array([100.0, 200.0, 3000.0]), np.arange(48) / 32.0
    z = p0 + v * t[:, None]
    c = _one_track(z, fps=32.0)
    assert np.array_equal(c['poses'][:, 0].astype(np.float64), z)
    p, vel, _, used, _ = TS.smooth_tracks(c['poses'], None, c['times'], c['rows'], c['starts'], mode, 'isotropic', q=4e6, r_floor=1.0,
                                         v0=1e8)
    first = 0 if mode == 'smooth' else 1
    err_p, err_v = np.abs(p[:, 0] - z).max(), np.abs(vel[first:, 0] - v).max()
    print(f'{mode}: worst position {err_p:.2e} mm, worst velocity {err_v:.2e} mm/s')
    assert used.all() and err_p <= 1e-6 and err_v <= 1e-3
    if mode == 'filter':
        assert (vel[0, 0] == 0).all()


@pytest.mark.parametrize('seed', range(20))
def test_synthetic_track_smoothed_beats_filtered_beats_raw(seed):
    """T = 48 at 30 fps, sinusoidal motion at 2 m depth, sigma = 10 mm with frame 20 declared (and drawn) at sigma = 150 mm,
    frames 30-33 missing, accel_psd = 4e6: over the measured frames after the fifth, RMS(smoothed) < RMS(filtered) < RMS(raw)."""
    rng = np.random.default_rng(seed)
    n = 48
    t = np.arange(n) / 30.0
    truth = np.stack([300 * np.sin(2 * np.pi * 0.5 * t), 100 * np.cos(2 * np.pi * 0.8 * t) + 50 * t, 2000 + 200 * t], axis=1)
    sig = np.full(n, 10.0)
    sig[20] = 150.0
    z = (truth + rng.normal(size=(n, 3)) * sig[:, None]).astype(np.float32)
    measured = np.ones(n, bool)
    measured[30:34] = False
    raw = z.copy()
    z[~measured] = np.nan
    cov = (sig[:, None, None] ** 2 * np.eye(3)[None]).reshape(n, 1, 9).astype(np.float32)
    c = _one_track(z, cov)
    out = {mode: TS.smooth_tracks(c['poses'], c['cov'], c['times'], c['rows'], c['starts'], mode, 'covariance', q=4e6, r_floor=1.0)
           for mode in MODES}
    m = measured & (np.arange(n) >= 5)
    rms = lambda a: np.sqrt(((a[m] - truth[m]) ** 2).sum(axis=1).mean())
    r_raw, r_filter, r_smooth = rms(raw.astype(np.float64)), rms(out['filter'][0][:, 0]), rms(out['smooth'][0][:, 0])
    print(f'seed {seed}: RMS raw {r_raw:.2f} mm, filtered {r_filter:.2f} mm, smoothed {r_smooth:.2f} mm')
    assert r_smooth < r_filter < r_raw
    assert np.array_equal(out['smooth'][3][:, 0] == 1, measured) and np.isfinite(out['smooth'][0]).all()


# ---- the kernel's own per-joint code on the host ------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def host_kernel(tmp_path_factory):
    """smooth_tracks.hip's per-joint function is __host__ __device__: the source compiled for the host, one call per (track,
    output joint) where the launch has one thread."""
    tmp = tmp_path_factory.mktemp('host_smooth_tracks')
    fn = compile_for_host(tmp, 'host_smooth_tracks', ['smooth_tracks.hip'], '''
extern "C" void host_smooth_tracks(const float* poses, const float* cov, const double* times, int n, const int* rows, int n_rows,
                                   const int* starts, int n_tracks, int n_out, int mode, int measurement, double q, double r_floor,
                                   double cov_scale, double v0, double gate, double* state, double* ws, float* poses_out,
                                   float* velocity_out, float* cov_out, unsigned char* used_out) {
    const metro::SmoothArgs a = metro::make_smooth_args(poses, cov, times, n, rows, n_rows, starts, n_tracks, n_out, mode, measurement,
                                                        q, r_floor, cov_scale, v0, gate, state, ws, poses_out, velocity_out, cov_out,
                                                        used_out);
    for (int idx = 0; idx < n_tracks * n_out; ++idx) metro::smooth_track_joint(a, idx);
}
''').host_smooth_tracks
    fn.restype = None
    fn.argtypes = ([C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 4 + [C.c_double] * 5 + [C.c_void_p] * 6)

    def run(c, state=None, **changes):
        """-> (poses, velocity, covariance, used), outputs pre-filled with the sentinel; `state` is updated in place."""
        c = {**c, **changes}
        n, nj = c['poses'].shape[:2]
        poses, vel, cov = (np.full((n, nj, k), TS.SENTINEL, np.float32) for k in (3, 3, 9))
        used = np.full((n, nj), int(abs(TS.SENTINEL)), np.uint8)
        ws = np.zeros(len(c['rows']) * nj * 54)
        times, rows, starts = (np.ascontiguousarray(c[k], d) for k, d in (('times', np.float64), ('rows', np.int32), ('starts', np.int32)))
        ptr = lambda a: C.c_void_p(a.ctypes.data if a is not None else 0)
        fn(ptr(np.ascontiguousarray(c['poses'])), ptr(c['cov']), ptr(times), n, ptr(rows), len(rows), ptr(starts), len(starts) - 1, nj,
           MH.SMOOTH_MODES[c['mode']], MH.SMOOTH_MEASUREMENTS[c['measurement']], c['q'], c['r_floor'], c['cov_scale'], c['v0'], c['gate'],
           ptr(state), ptr(ws), ptr(poses), ptr(vel), ptr(cov), ptr(used))
        return poses, vel, cov, used
    return run


@pytest.mark.parametrize('name', list(CASES))
@pytest.mark.parametrize('measurement', MEASUREMENTS)
@pytest.mark.parametrize('mode', MODES)
def test_kernel_code_on_the_host_matches_the_restatement(host_kernel, name, mode, measurement):
    """Positions within 1e-3 mm, velocities within 1e-3 mm/s, covariances within 1e-6 of their block's largest entry, `used`
    equal, rows in no group untouched, on every case of the helper."""
    c, want = TS.case_and_expected(name, mode, measurement)
    got = host_kernel(c)
    worst = TS.compare(got, want)
    print(f'{name}, {mode}, {measurement}: worst position {worst[0]:.2e} mm, velocity {worst[1]:.2e} mm/s, covariance {worst[2]:.2e} rel')
    TS.check_case(name, c, got)


def _chunk_case(mode, measurement):
    """One track of 24 rows (scrambled in memory), a second of 7 that ends inside the first chunk's time span."""
    c = TS.build([24, 7], 17, mode, measurement)
    c['poses'][TS._track_rows(c, 0)[12]] = np.nan
    return c


def _chunks(c, cut=10):
    """The case cut after `cut` rows of track 0: two (rows, starts) pairs; track 1 lies in the first chunk only."""
    r0, r1 = TS._track_rows(c, 0), TS._track_rows(c, 1)
    first = (np.concatenate([r0[:cut], r1]), np.asarray([0, cut, cut + len(r1)], np.int32))
    second = (r0[cut:], np.asarray([0, len(r0) - cut, len(r0) - cut], np.int32))
    return first, second


@pytest.mark.parametrize('measurement', MEASUREMENTS)
def test_chunked_filter_with_carried_state_is_one_call(host_kernel, measurement):
    """Filter mode on T = 24 cut 10 + 14 with the state carried equals one call bit for bit, outputs and final state; the track
    without rows in the second call keeps its slot; the restatement's state agrees."""
    c = _chunk_case('filter', measurement)
    fresh = lambda: np.full((2, TS.J, 28), np.nan)
    whole_state = fresh()
    whole = host_kernel(c, whole_state)
    state = fresh()
    (rows_a, starts_a), (rows_b, starts_b) = _chunks(c)
    a = host_kernel(c, state, rows=rows_a, starts=starts_a)
    kept = state[1].copy()
    b = host_kernel(c, state, rows=rows_b, starts=starts_b)
    for w, ga, gb in zip(whole, a, b):
        merged = ga.copy()
        merged[rows_b] = gb[rows_b]
        assert np.array_equal(merged, w, equal_nan=True)
    assert np.array_equal(state, whole_state) and np.isfinite(state).all() and np.array_equal(state[1], kept)
    assert np.array_equal(state[0, :, 27], np.full(TS.J, c['times'][TS._track_rows(c, 0)[-1]]))
    ref_state = TS.run_ref(c, fresh())[4]
    assert np.abs(state - ref_state).max() <= 1e-9 * np.abs(ref_state).max()
    # the carried state against the restatement: the second chunk from the first chunk's state
    want = TS.expected({**c, 'rows': rows_b, 'starts': starts_b}, TS.run_ref({**c, 'rows': rows_a, 'starts': starts_a}, fresh())[4])
    TS.compare(tuple(g[rows_b] for g in b), tuple(w[rows_b] for w in want))


@pytest.mark.parametrize('measurement', MEASUREMENTS)
def test_smooth_mode_ends_each_chunk_at_its_filtered_value(host_kernel, measurement):
    """In smooth mode the last row of a track in a call is its filtered value (bit for bit), the state written back is the filter
    state (never smoothed values), and earlier rows differ from the filter's."""
    c = _chunk_case('smooth', measurement)
    (rows_a, starts_a), _ = _chunks(c)
    s_smooth, s_filter = np.full((2, TS.J, 28), np.nan), np.full((2, TS.J, 28), np.nan)
    sm = host_kernel(c, s_smooth, rows=rows_a, starts=starts_a)
    fl = host_kernel(c, s_filter, rows=rows_a, starts=starts_a, mode='filter')
    assert np.array_equal(s_smooth, s_filter)
    for last in (rows_a[9], rows_a[-1]):
        for s, f in zip(sm, fl):
            assert np.array_equal(s[last], f[last])
    assert not np.array_equal(sm[0][rows_a[3]], fl[0][rows_a[3]]) and np.array_equal(sm[3], fl[3])
    # the smoothed position variance never exceeds the filtered one
    assert (sm[2][rows_a][..., [0, 4, 8]] <= fl[2][rows_a][..., [0, 4, 8]] * (1 + 1e-6)).all()


# ---- the Python surface ---------------------------------------------------------------------------------------------------------

def _naive_groups(ti, ts):
    groups = []
    for t in range(max(ti) + 1 if len(ti) else 0):
        mine = [i for i in range(len(ti)) if ti[i] == t]
        groups.append(sorted(mine, key=lambda i: ts[i]))
    return groups


@pytest.mark.parametrize('ti,ts', [
    ([0, 0, 0, 1, 1, 2], [0.0, 0.1, 0.2, 0.0, 0.1, 0.0]),                 # ragged, already in order
    ([2, 0, 1, 0, 2, 1, 2], [0.5, 0.4, 0.3, 0.2, 0.1, 0.0, 0.3]),          # unsorted in track and time
    ([3, 0, -1, 3, 0, 5, -1], [0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 1.0]),        # gaps (1, 2, 4) and untracked rows
    ([0, 1, 0, 1], [7.0, 7.0, 6.0, 8.0]),                                  # equal times on different tracks
    ([-1, -1], [0.0, 0.0]),                                                # nobody tracked: no groups
    ([], []),
], ids=['ragged', 'unsorted', 'gaps-untracked', 'equal-times', 'untracked', 'empty'])
def test_track_groups(ti, ts):
    rows, starts = FR.track_groups(ti, ts)
    want = _naive_groups(ti, ts)
    assert rows.dtype == np.int32 and starts.dtype == np.int32 and len(starts) == len(want) + 1
    assert starts[0] == 0 and starts[-1] == len(rows) == sum(t >= 0 for t in ti)
    assert [list(rows[starts[t]:starts[t + 1]]) for t in range(len(want))] == want


def test_track_groups_rejects_bad_input():
    with pytest.raises(ValueError, match='-1 for untracked'):
        FR.track_groups([0, -2], [0.0, 1.0])
    with pytest.raises(ValueError, match='holds 2 values'):
        FR.track_groups([0, 1], [0.0])
    for bad in (float('nan'), float('inf')):
        with pytest.raises(ValueError, match='finite'):
            FR.track_groups([0, 0], [0.0, bad])
    with pytest.raises(ValueError, match='two rows at the same time'):
        FR.track_groups([0, 1, 0], [0.5, 0.5, 0.5])


def test_new_track_state():
    s = FR.new_track_state(3, 17, 'cpu')
    assert s.shape == (3, 17, 28) and s.dtype == torch.float64 and torch.isnan(s[..., 27]).all() and (s[..., :27] == 0).all()


def test_python_surface_checks_arguments_without_a_gpu():
    sig = inspect.signature(FR.track_poses_in_frames)
    locate = [p for p in inspect.signature(FR.locate_poses_in_frames).parameters
              if p not in ('frames', 'boxes', 'model_path', 'cameras', 'frame_index', 'return_spread', 'return_uncertainty')]
    assert list(sig.parameters) == ['frames', 'boxes', 'model_path', 'cameras', 'track_index', 'frame_index', 'timestamps', 'state',
                                    'mode', 'measurement', 'accel_psd', 'sigma_floor_mm', 'cov_scale', 'initial_speed_mm_s',
                                    'gate'] + locate
    for name in locate:
        assert sig.parameters[name].default == inspect.signature(FR.locate_poses_in_frames).parameters[name].default
    d = {k: v.default for k, v in inspect.signature(MH.smooth_tracks).parameters.items()}
    assert list(d) == ['poses', 'covariance', 'times', 'rows', 'starts', 'mode', 'measurement', 'accel_psd', 'sigma_floor_mm',
                       'cov_scale', 'initial_speed_mm_s', 'gate', 'state']
    assert (d['mode'], d['measurement'], d['accel_psd'], d['sigma_floor_mm'], d['cov_scale'], d['initial_speed_mm_s'], d['gate'],
            d['state']) == ('smooth', 'covariance', 4e6, 1.0, 1.0, 2000.0, None, None)
    for k in ('state', 'mode', 'measurement', 'accel_psd', 'sigma_floor_mm', 'cov_scale', 'initial_speed_mm_s', 'gate'):
        assert sig.parameters[k].default == d[k]
    assert FR.TrackPoses._fields == ('poses', 'velocity', 'covariance', 'used', 'raw', 'state', 'joint_edges', 'joint_names')
    import metro_pose3d_amd
    assert metro_pose3d_amd.track_poses_in_frames is FR.track_poses_in_frames and 'track_poses_in_frames' in metro_pose3d_amd.__all__
    frames = [np.zeros((8, 8, 3), np.uint8)] * 2
    boxes = [[0, 0, 4, 4], [1, 1, 4, 4]]
    call = lambda ti=(0, 0), fi=(0, 1), ts=(0.0, 0.1), **kw: FR.track_poses_in_frames(frames, boxes, 'no-such-model.npz', None, ti, fi,
                                                                                      ts, **kw)
    for bad in ('rts', None, 1):
        with pytest.raises(ValueError, match='mode must be'):
            call(mode=bad)
    for bad in ('uniform', None):
        with pytest.raises(ValueError, match='measurement must be'):
            call(measurement=bad)
    for key in ('accel_psd', 'sigma_floor_mm', 'initial_speed_mm_s', 'gate'):
        for bad in (0, -1.0, float('nan'), float('inf'), '1', True):
            with pytest.raises(ValueError, match=key):
                call(**{key: bad})
    for bad in (-0.5, float('nan'), '1'):
        with pytest.raises(ValueError, match='cov_scale'):
            call(cov_scale=bad)
    with pytest.raises(ValueError, match='-1 for untracked'):
        call(ti=(0, -2))
    with pytest.raises(ValueError, match='one value per box'):
        call(ti=(0, 0, 0))
    with pytest.raises(ValueError, match='one value per box'):
        call(fi=(0,))
    with pytest.raises(ValueError, match='do not cover'):
        call(ts=(0.0,))                                    # one per frame, but frame 1 has none
    with pytest.raises(ValueError, match='finite'):
        call(ts=(0.0, float('nan')))
    with pytest.raises(ValueError, match='two rows at the same time'):
        call(ts=(0.5, 0.5))
    with pytest.raises(ValueError, match='different times'):
        call(fi=(0, 0), ts=(0.0, 0.1))
    with pytest.raises(ValueError, match='two rows at the same time'):
        call(fi=(1, 1), ts=(0.0, 0.1, 0.2))                # per frame: both boxes at frame 1's time
    for bad in (torch.zeros((2, 17, 28)), torch.zeros((1, 17, 27), dtype=torch.float64), torch.zeros((0, 17, 28), dtype=torch.float64)):
        with pytest.raises(ValueError, match='state must be'):
            call(state=bad)
    # heads.smooth_tracks: checked before the library or a device is touched
    n, nj = 4, 17
    poses, cov = torch.zeros((n, nj, 3)), torch.zeros((n, nj, 3, 3))
    run = lambda p=poses, c=cov, t=(0.0, 0.1, 0.2, 0.3), rows=(0, 1, 2, 3), starts=(0, 4), **kw: MH.smooth_tracks(p, c, t, rows, starts, **kw)
    with pytest.raises(ValueError, match='mode must be'):
        run(mode='backward')
    with pytest.raises(ValueError, match='measurement must be'):
        run(measurement='diag')
    with pytest.raises(ValueError, match='accel_psd'):
        run(accel_psd=0)
    with pytest.raises(ValueError, match='gate'):
        run(gate=-1)
    with pytest.raises(ValueError, match='poses must be'):
        run(p=poses[..., :2])
    with pytest.raises(ValueError, match='needs covariance'):
        run(c=None)
    with pytest.raises(ValueError, match='needs covariance'):
        run(c=cov[:3])
    with pytest.raises(ValueError, match='one value per pose row'):
        run(t=(0.0, 0.1))
    with pytest.raises(ValueError, match='starts'):
        run(starts=())
    with pytest.raises(ValueError, match='state must be'):
        run(state=torch.zeros((1, nj, 28)))
    with pytest.raises(ValueError, match='state must be'):
        run(state=torch.zeros((2, nj, 28), dtype=torch.float64))


def test_new_symbols_in_header_bindings_and_library(lib):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'metro_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(metro_[a-z0-9_]+)\s*\(', text))
    for name, n_args in (('metro_smooth_tracks', 23), ('metro_smooth_tracks_workspace_bytes', 2)):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
        params = re.search(r'\b' + name + r'\s*\(([^)]*)\)', text).group(1)
        assert len(_lib.SIGNATURES[name][1]) == params.count(',') + 1 == n_args
    for define, value in (('FILTER', 0), ('RTS', 1), ('ISOTROPIC', 0), ('COVARIANCE', 1)):
        assert re.search(rf'#define\s+METRO_SMOOTH_{define}\s+{value}\b', text) and getattr(_lib, f'METRO_SMOOTH_{define}') == value
    assert lib.metro_abi_version() == 8                    # the ABI is additive
    assert lib.metro_smooth_tracks_workspace_bytes(71, 17) == 71 * 17 * 54 * 8
    assert lib.metro_smooth_tracks_workspace_bytes(0, 17) == 0 and lib.metro_smooth_tracks_workspace_bytes(-1, 17) == 0


def test_c_entry_rejects_bad_arguments(lib):
    """Every return below comes before any launch: no device is needed."""
    cs = _lib.MetroSpec(n_joints_out=17)
    p = C.c_void_p(256)
    fn = lib.metro_smooth_tracks
    good = [p, p, p, 8, p, 8, p, 2, C.byref(cs), _lib.METRO_SMOOTH_RTS, _lib.METRO_SMOOTH_COVARIANCE, 4e6, 1.0, 1.0, 2000.0, 0.0,
            None, p, p, None, None, None, None]

    def call(**changes):
        a = list(good)
        for k, v in changes.items():
            a[int(k[1:])] = v
        return fn(*a)
    assert call(a8=None) == -1 and b'NULL spec' in lib.metro_last_error()
    for nj in (0, 65):
        assert call(a8=C.byref(_lib.MetroSpec(n_joints_out=nj))) == -1 and b'n_joints_out' in lib.metro_last_error()
    for bad in (-1, 2):
        assert call(a9=bad) == -1 and b'mode' in lib.metro_last_error()
        assert call(a10=bad) == -1 and b'measurement' in lib.metro_last_error()
    for k in (3, 5, 7):                                     # n, n_rows, n_tracks
        assert call(**{f'a{k}': -1}) == -1 and b'negative' in lib.metro_last_error()
    nan = float('nan')
    for k, word in ((11, b'q must'), (12, b'r_floor'), (14, b'v0')):
        for bad in (0.0, -1.0, nan):
            assert call(**{f'a{k}': bad}) == -1 and word in lib.metro_last_error()
    for k, word in ((13, b'cov_scale'), (15, b'gate')):
        for bad in (-1.0, nan):
            assert call(**{f'a{k}': bad}) == -1 and word in lib.metro_last_error()
    for k in (0, 2, 4, 6, 18):                              # poses, times, rows, starts, poses_out
        assert call(**{f'a{k}': None}) == -1 and b'NULL poses' in lib.metro_last_error()
    assert call(a1=None) == -1 and b'covariance: NULL' in lib.metro_last_error()
    assert call(a17=None) == -1 and b'workspace: NULL' in lib.metro_last_error()
    # nothing to do: no launch, whatever the pointers
    assert call(a7=0) == 0 and call(a5=0) == 0
    assert fn(None, None, None, 0, None, 0, None, 0, C.byref(cs), 0, 0, 4e6, 1.0, 0.0, 1.0, 0.0, None, None, None, None, None, None,
              None) == 0
