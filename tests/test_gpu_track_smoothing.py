"""metro_smooth_tracks, heads.smooth_tracks and frames.track_poses_in_frames on the MI355X: the launch against its fp64
restatement (tests/track_smoothing_ref.py) on the same fp32 inputs -- ragged and scrambled tracks across a block boundary,
gaps, late starts, bad covariances, skipped rows, a gated outlier, both modes and both measurement kinds -- the carried
state, and the whole call against locate_poses_in_frames plus heads.smooth_tracks.  Every GPU step runs once."""
import ctypes as C

import numpy as np
import pytest
import torch

from metro_pose3d_amd import _lib, frames as FR, heads as MH
from metro_pose3d_amd._lib import check
from tests import track_smoothing_ref as TS

pytestmark = pytest.mark.gpu

CASES, MODES, MEASUREMENTS, SENTINEL = TS.CASES, TS.MODES, TS.MEASUREMENTS, TS.SENTINEL


def _up(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _same(a, b):
    """torch.equal with NaN equal to NaN."""
    if not a.is_floating_point():
        return torch.equal(a, b)
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(nan=0.0), b.nan_to_num(nan=0.0))


def _launch(c, cuda):
    """One metro_smooth_tracks call into outputs pre-filled with the sentinel -> (poses, velocity, covariance, used) NumPy arrays."""
    n, nj = c['poses'].shape[:2]
    lib = _lib.load()
    poses, cov, times = _up(c['poses'], cuda), _up(c['cov'], cuda), _up(np.asarray(c['times'], np.float64), cuda)
    rows, starts = _up(np.asarray(c['rows'], np.int32), cuda), _up(np.asarray(c['starts'], np.int32), cuda)
    out, vel = (torch.full((n, nj, 3), SENTINEL, dtype=torch.float32, device=cuda) for _ in range(2))
    cov_out = torch.full((n, nj, 9), SENTINEL, dtype=torch.float32, device=cuda)
    used = torch.full((n, nj), int(abs(SENTINEL)), dtype=torch.uint8, device=cuda)
    ws = torch.empty(lib.metro_smooth_tracks_workspace_bytes(len(c['rows']), nj), dtype=torch.uint8, device=cuda)
    assert ws.numel() == len(c['rows']) * nj * 54 * 8
    cs = _lib.MetroSpec(n_joints_out=nj)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    check(lib.metro_smooth_tracks(ptr(poses), ptr(cov), ptr(times), n, ptr(rows), len(c['rows']), ptr(starts), len(c['starts']) - 1,
                                  C.byref(cs), MH.SMOOTH_MODES[c['mode']], MH.SMOOTH_MEASUREMENTS[c['measurement']], c['q'], c['r_floor'],
                                  c['cov_scale'], c['v0'], c['gate'], None, ptr(ws), ptr(out), ptr(vel), ptr(cov_out), ptr(used),
                                  C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)), 'metro_smooth_tracks')
    return out.cpu().numpy(), vel.cpu().numpy(), cov_out.cpu().numpy(), used.cpu().numpy()


@pytest.mark.parametrize('name', list(CASES))
@pytest.mark.parametrize('measurement', MEASUREMENTS)
@pytest.mark.parametrize('mode', MODES)
def test_kernel_matches_the_restatement(cuda, name, mode, measurement):
    """Positions within 1e-3 mm and velocities within 1e-3 mm/s of the restatement rounded to fp32 (both sides fp64 on
    identical fp32 inputs; one fp32 rounding below 8192 is <= 4.9e-4), covariances within 1e-6 of their block's largest entry,
    `used` equal, equal NaN pattern; rows in no group keep the sentinel in all four outputs; then what the case is there to
    show (TS.check_case).  threads272 is 16 tracks x 17 joints: across the 256-thread block."""
    c, want = TS.case_and_expected(name, mode, measurement)
    got = _launch(c, cuda)
    worst = TS.compare(got, want)
    print(f'{name}, {mode}, {measurement}: worst position {worst[0]:.2e} mm, velocity {worst[1]:.2e} mm/s, covariance {worst[2]:.2e} rel '
          'vs the fp64 restatement')
    TS.check_case(name, c, got)


def test_binding_is_the_launch_and_fills_rows_in_no_group(cuda):
    """heads.smooth_tracks returns the launch's bits on listed rows; rows in no group come back with their input pose, NaN
    velocity, their R and used 0; a one-row track returns its input pose bits."""
    c, _ = TS.case_and_expected('ragged', 'smooth', 'covariance')
    got = _launch(c, cuda)
    poses, cov = _up(c['poses'], cuda), _up(c['cov'], cuda)
    out = MH.smooth_tracks(poses, cov.view(-1, TS.J, 3, 3), c['times'], c['rows'], c['starts'], c['mode'], c['measurement'], c['q'],
                           c['r_floor'], c['cov_scale'], c['v0'], None)
    assert out[2].shape == (len(poses), TS.J, 3, 3) and out[3].dtype == torch.uint8 and out[0].device.type == 'cuda'
    listed = np.zeros(len(poses), bool)
    listed[c['rows']] = True
    for a, b in zip(out, got):
        assert np.array_equal(a.cpu().numpy().reshape(b.shape)[listed], b[listed], equal_nan=True)
    rest = torch.from_numpy(~listed).to(cuda)
    assert rest.any() and torch.equal(out[0][rest], poses[rest]) and torch.isnan(out[1][rest]).all() and not out[3][rest].any()
    want_r = torch.from_numpy(np.stack([TS.measurement_noise(c['cov'][i, j], 'covariance', c['r_floor'], c['cov_scale'])
                                        for i in np.flatnonzero(~listed) for j in range(TS.J)]).astype(np.float32)).to(cuda)
    assert torch.allclose(out[2][rest].reshape(-1, 3, 3), want_r, rtol=1e-6, atol=0)
    one = int(TS._track_rows(c, 0)[0])
    assert torch.equal(out[0][one], poses[one]) and (out[1][one] == 0).all() and out[3][one].all()


@pytest.mark.parametrize('measurement', MEASUREMENTS)
def test_chunked_filter_with_carried_state_is_one_call(cuda, measurement):
    """Filter mode on T = 24 cut 10 + 14 with the state carried equals one call bit for bit, outputs and final state; in smooth
    mode a chunk's last row equals its filtered value and the state is the filter's."""
    c = TS.build([24, 7], 17, 'filter', measurement)
    r0, r1 = TS._track_rows(c, 0), TS._track_rows(c, 1)
    c['poses'][r0[12]] = np.nan
    poses, cov = _up(c['poses'], cuda), _up(c['cov'], cuda)
    run = lambda rows, starts, state, mode='filter': MH.smooth_tracks(poses, cov, c['times'], rows, starts, mode, measurement, c['q'],
                                                                      c['r_floor'], c['cov_scale'], c['v0'], None, state)
    whole_state, state, smooth_state = (FR.new_track_state(2, TS.J, cuda) for _ in range(3))
    whole = run(c['rows'], c['starts'], whole_state)
    rows_a, starts_a = np.concatenate([r0[:10], r1]), [0, 10, 10 + len(r1)]
    a = run(rows_a, starts_a, state)
    after_a = state.clone()
    sm = run(rows_a, starts_a, smooth_state, 'smooth')
    b = run(r0[10:], [0, 14, 14], state)
    idx_b = torch.from_numpy(np.asarray(r0[10:], np.int64)).to(cuda)
    idx_a = torch.from_numpy(np.asarray(rows_a, np.int64)).to(cuda)
    for w, ga, gb in zip(whole, a, b):
        assert _same(ga[idx_a], w[idx_a])
        assert _same(gb[idx_b], w[idx_b])
    assert torch.equal(state, whole_state) and torch.isfinite(state).all() and torch.equal(state[1], after_a[1])
    assert torch.equal(smooth_state, after_a)
    for last in (int(rows_a[9]), int(rows_a[-1])):
        for s, f in zip(sm, a):
            assert _same(s[last], f[last])
    assert not torch.equal(sm[0][int(rows_a[3])], a[0][int(rows_a[3])])


def test_track_poses_in_frames_is_locate_plus_one_launch(cuda, tmp_path):
    """2 tracks x 3 frames, a third track with one box and an untracked box, crop_dtype and precision at their defaults: `raw` is
    locate_poses_in_frames(..., return_uncertainty=True) bit for bit, the smoothed outputs are heads.smooth_tracks on `raw`
    bit for bit, the one-row track returns its input pose bits, the untracked box its raw pose; a second call continues from
    the returned state."""
    from tests.test_gpu_placement import _toy_engine_model
    spec, _, path = _toy_engine_model(tmp_path)
    rng = np.random.default_rng(5)
    frames = [rng.integers(0, 256, (240, 320, 3), dtype=np.uint8) for _ in range(3)]
    boxes = np.array([[60.0, 40, 70, 150], [170, 50, 80, 140], [64, 42, 70, 150], [174, 52, 80, 140], [68, 44, 70, 150],
                      [178, 54, 80, 140], [10, 10, 60, 100], [200, 20, 60, 100]])
    fi, ti = np.array([0, 0, 1, 1, 2, 2, 1, 2]), np.array([0, 1, 0, 1, 0, 1, 2, -1])
    stamps = [0.0, 1 / 30, 2 / 30]                          # one per frame
    kw = dict(cameras=None, frame_index=fi, scale_recovery='metro')
    got = FR.track_poses_in_frames(frames, boxes, path, None, ti, fi, stamps, scale_recovery='metro')
    ref = FR.locate_poses_in_frames(frames, boxes, path, return_uncertainty=True, **kw)
    n_out = spec.skeleton.n_out
    assert got.poses.shape == (8, n_out, 3) and got.state.shape == (3, n_out, 28) and got.state.dtype == torch.float64
    for a, b in zip((got.raw.poses, got.raw.keypoints2d, got.raw.covariance, got.raw.peak), (ref.poses, ref.keypoints2d, ref.covariance, ref.peak)):
        assert torch.equal(a, b)
    assert got.raw.z_offset is None and len(got.joint_names) == n_out and got.joint_edges.shape[1] == 2
    rows, starts = FR.track_groups(ti, np.asarray(stamps)[fi])
    assert list(starts) == [0, 3, 6, 7]
    state = FR.new_track_state(3, n_out, cuda)
    want = MH.smooth_tracks(got.raw.poses, got.raw.covariance, np.asarray(stamps)[fi], rows, starts, state=state)
    for a, b in zip((got.poses, got.velocity, got.covariance, got.used), want):
        assert _same(a, b)
    assert torch.equal(got.state, state) and torch.isfinite(got.state).all()
    assert torch.equal(got.poses[6], got.raw.poses[6]) and got.used[6].all() and (got.velocity[6] == 0).all()
    assert torch.equal(got.poses[7], got.raw.poses[7]) and torch.isnan(got.velocity[7]).all() and not got.used[7].any()
    assert got.used[:6].all() and torch.isfinite(got.poses).all() and not torch.equal(got.poses[0], got.raw.poses[0])
    # the next call of the stream continues from the state, which it updates in place
    nxt = FR.track_poses_in_frames(frames[:1], boxes[:2], path, None, [0, 1], [0, 0], [3 / 30], state=got.state, mode='filter',
                                   scale_recovery='metro')
    assert nxt.state is got.state and (nxt.state[:2, :, 27] == 3 / 30).all() and (nxt.state[2, :, 27] == 1 / 30).all()
    assert nxt.used.all() and torch.isfinite(nxt.velocity).all()
