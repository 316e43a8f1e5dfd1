"""Track-predicted heat-map priors without a GPU: the fp64 restatement (tests/track_prior_ref.py) on known answers, the kernel's
own per-joint code (csrc/track_priors.hip) compiled for the host against that restatement at every shape at which a loop or a
block ends, the round trip with the back-projection the placement launch is made of, the chain restatement -> posterior
restatement on the two-peaked joint the feature exists for, the margins that keep every compared case away from a decision the
tolerance could flip, and the new C symbol in header, bindings and library with its refusals.

Bounds (track_prior_ref): both sides compute in fp64 and round once to fp32, so the reason words are equal, mu is within
2.4e-7 max(1, |mu|) and each precision block within 1e-6 of its largest entry."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from metro_pose3d_amd import ModelSpec, _lib, heads as MH
from metro_pose3d_amd._lib import MetroTrackPrior
from tests import heat_posterior_ref as PR
from tests import track_prior_ref as TP
from tests.helpers import compile_for_host
from tests.test_heat_posterior import gaussian_logits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECS = {'h36m': ModelSpec(50, 32, 'h36m'), 'many19': ModelSpec(50, 16, 'many19'),
         'merged': ModelSpec(50, 32, 'merged', centered_stride=False, proc_side=224)}
H36M = TP.Head(SPECS['h36m'])


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    """csrc/track_priors.hip's per-joint function on the host, one call per (row, joint) in the kernel's order of indices, and the
    back-projection of place_poses_kernel's absolute modes built from the camera_math.h functions it is built from."""
    lib = compile_for_host(tmp_path_factory.mktemp('track_prior_host'), 'host_track_priors', ['track_priors.hip'], '''
extern "C" void host_track_priors(const double* state, int capacity, const int* slot, const double* times, const MetroPlacement* rec,
                                  const int* mirror, const MetroTrackPrior* params, const float* coords01, int n, const MetroSpec* spec,
                                  float* prior, int* reason) {
    using namespace metro;
    const TrackPriorArgs a = make_track_prior_args(state, capacity, slot, times, rec, mirror, *params, coords01, n, *spec, prior, reason);
    for (int idx = 0; idx < n * a.n_out; ++idx) track_prior_one(a, idx);
}
// place_poses_kernel's back_project of one joint: crop_pixel, ray_through, the ray times its depth, rotate3, + cam_loc (fp32)
extern "C" void host_back_project(const float* c01, const MetroPlacement* rec, float lrc, float half_off, float depth, int world, float* out) {
    using namespace metro;
    float u, v, ray[3], x[3];
    crop_pixel(c01, lrc, half_off, u, v);
    ray_through(rec->inv_intrinsics, u, v, ray);
    for (int t = 0; t < 3; ++t) x[t] = ray[t] * depth;
    rotate3(world ? rec->rot_to_world : rec->rot_to_orig_cam, x, out);
    if (world) for (int t = 0; t < 3; ++t) out[t] = out[t] + rec->cam_loc[t];
}
''')
    lib.host_track_priors.restype = None
    lib.host_track_priors.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(MetroTrackPrior),
                                      C.c_void_p, C.c_int, C.POINTER(_lib.MetroSpec), C.c_void_p, C.c_void_p]
    lib.host_back_project.restype = None
    lib.host_back_project.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_int, C.c_void_p]
    return lib


def run_host(host, case):
    """The host-compiled kernel code on a restatement case -> (prior float32 [n, Jout, 9], reason int32 [n, Jout])."""
    head = case['head']
    n = len(case['slot'])
    state = np.ascontiguousarray(case['state'], np.float64)
    slot = np.ascontiguousarray(case['slot'], np.int32)
    times = np.ascontiguousarray(case['times'], np.float64)
    rec = np.ascontiguousarray(case['records'])
    mirror = np.ascontiguousarray(head.mirror, np.int32)
    c01 = np.ascontiguousarray(case['coords01'], np.float32)
    params = MH.track_prior_params(case['coords'], case['depth'], **dict(TP.DEFAULTS, **case.get('params', {})))
    prior = np.full((n, head.n_out, 9), -7.0, np.float32)
    reason = np.full((n, head.n_out), -7, np.int32)
    ptr = lambda a: a.ctypes.data
    host.host_track_priors(ptr(state), len(state), ptr(slot), ptr(times), ptr(rec), ptr(mirror), C.byref(params), ptr(c01), n,
                           C.byref(head.cspec), ptr(prior), ptr(reason))
    return prior, reason


def one_joint(x, p6=None, t_last=0.0, t=0.0, k=None, rot=None, coords='camera', depth='none', params=None, head=H36M, joint=0,
              slot=0, n_tracks=1, root=None, coords01=None, cam_loc=(0, 0, 0)):
    """A case of one row whose slot holds one joint (and, for depth 'root', the root): -> the case."""
    state = TP.empty_state(n_tracks, head.n_out)
    p6 = np.diag([50.0 ** 2] * 3 + [300.0 ** 2] * 3) if p6 is None else p6
    if 0 <= slot < n_tracks:
        state[slot, joint] = TP.pack_state(np.asarray(x, np.float64), p6, t_last)
        if root is not None:
            state[slot, head.root_out] = TP.pack_state(np.asarray(root, np.float64), p6, t_last)
    records = np.zeros(1, TP.PLACEMENT)
    records[0] = TP.record(TP.pinhole() if k is None else k, rot, None, cam_loc)
    c01 = np.full((1, head.n_head, 3), 0.5, np.float32) if coords01 is None else coords01
    return dict(head=head, state=state, slot=np.array([slot], np.int32), times=np.array([t]), records=records, coords=coords,
                depth=depth, params=dict(TP.DEFAULTS, **(params or {})), coords01=c01)


# ---- the restatement on known answers (and the kernel's code on the same) ------------------------------------------------------

def both(host, case):
    """The restatement's rows, after holding the host-compiled code to them."""
    prior, reason, _ = TP.prior(case)
    TP.check(*run_host(host, case), prior, reason)
    return prior.astype(np.float64), reason


def test_jacobian_against_central_differences():
    rng = np.random.default_rng(5)
    k = TP.pinhole(610.0, 127.0)
    k[0, 1] = 1.5
    for _ in range(8):
        c = np.array([rng.uniform(-800, 800), rng.uniform(-800, 800), rng.uniform(2500, 6000)])
        num = np.stack([(TP.project(c + h, k, H36M) - TP.project(c - h, k, H36M)) / 2.0 for h in np.eye(3)], 1)     # step 1 mm
        jac = TP.jacobian(c, k, H36M)
        assert np.abs(num - jac).max() <= 1e-6 * np.abs(jac).max(), (c, num, jac)


def test_joint_on_the_optical_axis(host):
    """mu is the principal point in heat-map units and L_xy = (z lrc / (f sigma))^2 I."""
    f, z, sigma = 550.0, 4500.0, 40.0
    p6 = np.diag([sigma ** 2] * 3 + [250.0 ** 2] * 3)
    prior, reason = both(host, one_joint([0, 0, z, 0, 0, 0], p6, params=dict(sigma_floor_mm=0.0)))
    assert reason[0, 0] == TP.GIVEN and (reason[0, 1:] == TP.NO_STATE).all() and (prior[0, 1:] == 0).all()
    mu = (128.0 - H36M.half) / H36M.lrc
    lxy = (z * H36M.lrc / (f * sigma)) ** 2
    assert np.abs(prior[0, 0, :2] - mu).max() < 1e-6
    assert np.abs(prior[0, 0, [3, 4]] - lxy).max() < 1e-6 * lxy and abs(prior[0, 0, 6]) < 1e-6 * lxy
    assert (prior[0, 0, [2, 5, 7, 8]] == 0).all(), 'depth none: no knowledge along z'


def test_velocity_moves_mu_and_sigma_grows_by_the_closed_form(host):
    f, z, v, dt, q = 550.0, 4500.0, 900.0, 0.25, 4e6
    sp, sv, pv = 40.0 ** 2, 300.0 ** 2, 2000.0
    p6 = np.diag([sp] * 3 + [sv] * 3)
    p6[0, 3] = p6[3, 0] = pv
    still, _ = both(host, one_joint([0, 0, z, 0, 0, 0], p6, t=dt, params=dict(sigma_floor_mm=0.0)))
    moved, _ = both(host, one_joint([0, 0, z, v, 0, 0], p6, t=dt, params=dict(sigma_floor_mm=0.0)))
    assert abs((moved[0, 0, 0] - still[0, 0, 0]) - f * v * dt / (z * H36M.lrc)) < 1e-6
    assert abs(moved[0, 0, 1] - still[0, 0, 1]) < 1e-7
    # the constant-velocity model: var_x(dt) = P_xx + 2 dt P_xv + dt^2 P_vv + q dt^3 / 3; var_y has no cross term here
    scale = (f / (z * H36M.lrc)) ** 2
    var_x = sp + 2 * dt * pv + dt * dt * sv + q * dt ** 3 / 3
    var_y = sp + dt * dt * sv + q * dt ** 3 / 3
    assert abs(1 / still[0, 0, 3] - scale * var_x) < 1e-6 * scale * var_x and abs(1 / still[0, 0, 4] - scale * var_y) < 1e-6 * scale * var_y
    wider, _ = both(host, one_joint([0, 0, z, 0, 0, 0], p6, t=2 * dt, params=dict(sigma_floor_mm=0.0)))
    assert wider[0, 0, 3] < still[0, 0, 3], 'the prior loosens with dt'
    early, _ = both(host, one_joint([0, 0, z, v, 0, 0], p6, t_last=1.0, t=0.5, params=dict(sigma_floor_mm=0.0)))
    rest, _ = both(host, one_joint([0, 0, z, v, 0, 0], p6, t_last=1.0, t=1.0, params=dict(sigma_floor_mm=0.0)))
    assert np.array_equal(early, rest), 'a row before the state: dt = max(t - t_last, 0) = 0'


def test_floor_and_scale_enter_the_covariance(host):
    z, f = 4500.0, 550.0
    p6 = np.diag([40.0 ** 2] * 3 + [0.0] * 3)
    prior, _ = both(host, one_joint([0, 0, z, 0, 0, 0], p6, params=dict(sigma_floor_mm=30.0, cov_scale=2.0, accel_psd=1e-9)))
    var = 2.0 * 40.0 ** 2 + 30.0 ** 2
    assert abs(1 / prior[0, 0, 3] - (f / (z * H36M.lrc)) ** 2 * var) < 1e-6 / prior[0, 0, 3]


def test_flipped_view_reads_the_mirror_joint(host):
    head = H36M
    r = next(r for r in range(head.n_out) if head.mirror[r] != r)
    flip = np.diag([-1.0, 1.0, 1.0])
    case = one_joint([300.0, -200.0, 4500.0, 0, 0, 0], joint=head.mirror[r], rot=flip)
    prior, reason = both(host, case)
    assert reason[0, r] == TP.GIVEN and reason[0, head.mirror[r]] == TP.NO_STATE
    # the flipped camera sees x mirrored: the pixel is left of the principal point
    assert abs(prior[0, r, 0] - (128.0 - 550.0 * 300.0 / 4500.0 - head.half) / head.lrc) < 1e-6
    plain, reason = both(host, one_joint([300.0, -200.0, 4500.0, 0, 0, 0], joint=head.mirror[r]))
    assert reason[0, head.mirror[r]] == TP.GIVEN and reason[0, r] == TP.NO_STATE
    assert abs(plain[0, head.mirror[r], 0] - (128.0 + 550.0 * 300.0 / 4500.0 - head.half) / head.lrc) < 1e-6


@pytest.mark.parametrize('what,kw,word', [
    ('slot -1', dict(slot=-1), TP.NO_SLOT),
    ('slot T', dict(slot=3, n_tracks=3), TP.NO_SLOT),
    ('a state with NaN t_last', dict(t_last=float('nan')), TP.NO_STATE),
    ('an age just past max_age_s', dict(t_last=2.0, t=3.0 + 1e-9), TP.TOO_OLD),
    ('a joint at near_mm - eps', dict(x=[0, 0, 100.0 - 1e-9, 0, 0, 0]), TP.NEAR),
    ('a joint behind the camera', dict(x=[0, 0, -4500.0, 0, 0, 0]), TP.NEAR),
    ('a NaN time', dict(t=float('nan')), TP.NONFINITE),
    ('a NaN position', dict(x=[float('nan'), 0, 4500.0, 0, 0, 0]), TP.NONFINITE),
    ('a covariance that is not invertible', dict(p6=np.zeros((6, 6)), params=dict(sigma_floor_mm=0.0, cov_scale=1.0, accel_psd=1e-300)),
     TP.SINGULAR),
])
def test_rows_without_a_prior(host, what, kw, word):
    kw = dict(dict(x=[0, 0, 4500.0, 0, 0, 0]), **kw)
    case = one_joint(**kw)
    ref_prior, ref_reason, _ = TP.prior(case)
    prior, reason = run_host(host, case)
    assert ref_reason[0, 0] == word and reason[0, 0] == word, (what, ref_reason[0, 0], reason[0, 0])
    assert np.array_equal(reason, ref_reason) and (prior == 0).all() and (ref_prior == 0).all(), what


def test_the_thresholds_themselves_give_a_prior(host):
    """An age of exactly max_age_s and a joint exactly at near_mm are inside."""
    for kw in (dict(t_last=2.0, t=3.0), dict(x=[0, 0, 100.0, 0, 0, 0])):
        case = one_joint(**dict(dict(x=[0, 0, 4500.0, 0, 0, 0]), **kw))
        assert TP.prior(case)[1][0, 0] == TP.GIVEN and run_host(host, case)[1][0, 0] == TP.GIVEN


def test_depth_relative_to_the_root(host):
    head = H36M
    r = next(r for r in range(head.n_out) if r != head.root_out)
    sp = 50.0 ** 2
    c01 = np.full((1, head.n_head, 3), 0.5, np.float32)
    c01[0, head.n_head - 1, 2] = 0.4375
    case = one_joint([100.0, 50.0, 4800.0, 0, 0, 0], joint=r, root=[0, 0, 4500.0, 0, 0, 0], depth='root', coords01=c01,
                     params=dict(sigma_floor_mm=0.0))
    prior, reason = both(host, case)
    assert reason[0, r] == TP.GIVEN and reason[0, head.root_out] == TP.GIVEN
    assert abs(prior[0, r, 2] - (0.4375 + 300.0 / head.box)) < 1e-7, 'a joint 300 mm behind the root'
    assert abs(prior[0, r, 5] - head.box ** 2 / (2 * sp)) < 1e-6 * head.box ** 2 / (2 * sp)
    assert (prior[0, r, 7:] == 0).all() and (prior[0, head.root_out, [2, 5, 7, 8]] == 0).all(), 'the root row has a zero z block'
    assert prior[0, head.root_out, 3] > 0
    none, _ = both(host, dict(case, depth='none'))
    assert (none[0, r, [2, 5]] == 0).all() and np.array_equal(none[0, r, [0, 1, 3, 4, 6]], prior[0, r, [0, 1, 3, 4, 6]])
    lone = one_joint([100.0, 50.0, 4800.0, 0, 0, 0], joint=r, depth='root', coords01=c01)
    prior, reason = both(host, lone)
    assert reason[0, r] == TP.GIVEN and (prior[0, r, [2, 5]] == 0).all(), 'no root state: xy only'


# ---- round trip with the back-projection of the placement -----------------------------------------------------------------------

@pytest.mark.parametrize('coords', ['camera', 'world'])
def test_round_trip_with_the_placement(host, coords):
    """Joints the placement's own back-projection (its fp32 code, compiled for the host) placed from a coords01, stored as a track
    state with dt = 0, come back as mu_xy = coords01.xy within 1e-6: the projection is the inverse of the back-projection the
    project already trusts."""
    head, world = H36M, coords == 'world'
    rng = np.random.default_rng(11)
    worst = 0.0
    for trial in range(6):
        orig_r = TP.rotation(rng, 0.8) if world else np.eye(3)
        virt = TP.rotation(rng, 0.3) @ (np.diag([-1.0, 1.0, 1.0]) if trial % 3 == 2 else np.eye(3))
        rec = np.zeros(1, TP.PLACEMENT)
        rec[0] = TP.record(TP.pinhole(rng.uniform(400, 700)), orig_r.T @ virt, orig_r, rng.uniform(-2000, 2000, 3) if world else (0, 0, 0))
        flipped = trial % 3 == 2
        c01 = rng.uniform(0.05, 0.95, (1, head.n_head, 3)).astype(np.float32)
        state = TP.empty_state(1, head.n_out)
        for r in range(head.n_out):
            j = head.perm[head.mirror[r] if flipped else r]           # to_orig_cam: a flipped view's row r holds its mirror joint
            out = np.zeros(3, np.float32)
            host.host_back_project(c01[0, j].ctypes.data, rec.ctypes.data, head.lrc, head.half, float(rng.uniform(3000, 6000)), int(world),
                                   out.ctypes.data)
            state[0, r] = TP.pack_state(np.concatenate([out.astype(np.float64), rng.uniform(-500, 500, 3)]), TP.random_cov6(rng), 2.0)
        case = dict(head=head, state=state, slot=np.zeros(1, np.int32), times=np.array([2.0]), records=rec, coords=coords, depth='none',
                    params=dict(TP.DEFAULTS), coords01=c01)
        prior, reason = both(host, case)
        assert (reason == TP.GIVEN).all()
        # row r of the prior is head joint perm[r] of the crop as the network sees it, which is where row mirror[r] of the table lies
        err = np.abs(prior[0, :, :2] - c01[0, head.perm, :2].astype(np.float64)).max()
        worst = max(worst, err)
    print(f'round trip {coords}: worst |mu_xy - coords01.xy| {worst:.3e} (bound 1e-6)')
    assert worst < 1e-6


# ---- what it is for, on the restatements alone ------------------------------------------------------------------------------------

def test_track_at_the_weaker_peak_moves_the_posterior_onto_it():
    """The 0.55 / 0.45 two-peak volume of tests/test_heat_posterior.py: a track that predicts the joint at the weaker peak moves
    the posterior mean onto it; a free slot leaves the plain mean."""
    head = H36M
    s, d, sig = 16, 8, np.array([0.06, 0.06, 0.11])
    vol = np.log(0.55 * np.exp(gaussian_logits(s, d, (0.30, 0.5, 0.5), sig)) + 0.45 * np.exp(gaussian_logits(s, d, (0.70, 0.5, 0.5), sig)))
    # the point of the crop's camera that projects to heat-map (0.70, 0.5), 4.5 m away
    k = TP.pinhole()
    z = 4500.0
    uv = np.array([0.70, 0.5]) * head.lrc + head.half
    x = np.array([(uv[0] - k[0, 2]) / k[0, 0] * z, (uv[1] - k[1, 2]) / k[1, 1] * z, z])
    p6 = np.diag([60.0 ** 2] * 3 + [300.0 ** 2] * 3)
    for slot, lands in ((0, 0.70), (-1, None)):
        case = one_joint(np.concatenate([x, np.zeros(3)]), p6, slot=slot, t=0.02)
        prior, reason, _ = TP.prior(case)
        assert reason[0, 0] == (TP.GIVEN if slot == 0 else TP.NO_SLOT)
        post = PR.posterior(vol.reshape(1, s, s, d), 1, d, [0], prior[:, :1].astype(np.float64))[0, 0]
        plain = PR.posterior(vol.reshape(1, s, s, d), 1, d, [0], np.zeros((1, 1, 9)))[0, 0]
        if lands is None:
            assert post[0] == 0.0 and np.array_equal(post, plain) and 0.47 <= post[2] <= 0.49
        else:
            assert abs(prior[0, 0, 0] - 0.70) < 1e-6 and abs(prior[0, 0, 1] - 0.5) < 1e-6
            assert abs(post[2] - lands) < 0.01 and np.sqrt(post[5]) < 0.06 and post[0] < 0
            # a Gaussian peak of sd 0.06 under a centred Gaussian prior of sd sp, per axis: sp / sqrt(0.06^2 + sp^2); the grid of 16
            # points (step 0.067) stands for the integral to a few per cent
            sp = 550.0 * np.hypot(60.0, 30.0) / (z * head.lrc)
            assert abs(np.exp(post[0]) / (0.45 * sp ** 2 / (0.06 ** 2 + sp ** 2)) - 1) < 0.1, 'the mass of the weaker peak the prior covers'


# ---- the kernel's code against the restatement at every boundary ----------------------------------------------------------------

def merged_head():
    return TP.Head(SPECS['merged'])


SHAPES = [
    # rows (64 (row, joint) pairs a block), output joints, T, coords, depth, views
    (1, 'one', 1, 'camera', 'none', 1), (1, 'h36m', 1, 'camera', 'root', 1), (63, 'one', 128, 'world', 'none', 1),
    (64, 'one', 128, 'camera', 'none', 1), (65, 'one', 1, 'world', 'none', 1), (63, 'h36m', 128, 'world', 'root', 3),
    (64, 'many19', 128, 'camera', 'root', 1), (65, 'merged', 128, 'world', 'none', 1), (255, 'h36m', 128, 'camera', 'none', 3),
    (256, 'many19', 1, 'world', 'root', 1), (256, 'merged', 128, 'camera', 'root', 1), (255, 'merged', 128, 'world', 'root', 3),
]


def head_of(name):
    return TP.Head(SPECS['h36m'], n_out=1) if name == 'one' else TP.Head(SPECS[name])


@pytest.mark.parametrize('n,joints,n_tracks,coords,depth,views', SHAPES)
def test_host_compiled_code_against_the_restatement(host, n, joints, n_tracks, coords, depth, views):
    head = head_of(joints)
    if depth == 'root' and head.root_out < 0:
        depth = 'none'                                  # the merged output order has no root: the bind refuses 'root' there
    rows = n - n % views if n >= views else views       # whole boxes
    case = TP.random_case(head, rows, n_tracks, coords, depth, views, seed=3)
    ref_prior, ref_reason, margins = TP.prior(case)
    TP.check_margins(margins, (n, joints))
    prior, reason = run_host(host, case)
    TP.check(prior, reason, ref_prior, ref_reason, f'n {rows} J {head.n_out} T {n_tracks} {coords} {depth} V {views}')
    present = {int(w) for w in np.unique(ref_reason)}
    assert TP.GIVEN in present
    if rows >= 63:
        assert {TP.NO_SLOT, TP.GIVEN} <= present, present
    if rows >= 255 and head.n_out > 1:
        assert {TP.NO_SLOT, TP.NO_STATE, TP.TOO_OLD, TP.NEAR, TP.NONFINITE} <= present, present
    if views > 1:
        rot = case['records']['rot_to_world' if coords == 'world' else 'rot_to_orig_cam'].astype(np.float64).reshape(-1, 3, 3)
        assert (np.linalg.det(rot) < 0).sum() == rows // views, 'one flipped view per box'


def test_merged_output_order_has_no_root():
    assert merged_head().root_out == -1 and H36M.root_out >= 0 and head_of('many19').root_out >= 0


def test_margin_check_refuses_a_case_on_a_threshold():
    for kw in (dict(t_last=2.0, t=3.0 + 1e-4), dict(x=[0, 0, 100.05, 0, 0, 0])):
        margins = TP.prior(one_joint(**dict(dict(x=[0, 0, 4500.0, 0, 0, 0]), **kw)))[2]
        with pytest.raises(AssertionError):
            TP.check_margins(margins)
    narrow = np.diag([1.0, 300.0 ** 2, 1.0, 1.0, 1.0, 1.0])
    margins = TP.prior(one_joint([0, 0, 4500.0, 0, 0, 0], narrow, params=dict(sigma_floor_mm=0.0, accel_psd=1e-9)))[2]
    assert margins['cond'] > TP.MAX_COND
    with pytest.raises(AssertionError):
        TP.check_margins(margins)


# ---- the Python surface before any device is touched ---------------------------------------------------------------------------

def test_track_prior_params_validates_the_keywords():
    p = MH.track_prior_params()
    assert (p.coords, p.depth) == (_lib.METRO_COORDS_CAMERA, _lib.METRO_TRACK_PRIOR_DEPTH_NONE)
    assert (p.accel_psd, p.max_age_s, p.near_mm, p.sigma_floor_mm, p.cov_scale) == (4e6, 1.0, 100.0, 30.0, 1.0)
    assert MH.track_prior_params('world', 'root').depth == _lib.METRO_TRACK_PRIOR_DEPTH_ROOT
    for bad in (dict(coords='crop'), dict(depth='z'), dict(accel_psd=0.0), dict(max_age_s=-1.0), dict(near_mm=0.0),
                dict(sigma_floor_mm=float('nan')), dict(cov_scale=-1.0), dict(cov_scale=True), dict(sigma_floor_mm=0.0, cov_scale=0.0),
                dict(max_age_s=float('inf'))):
        with pytest.raises(ValueError):
            MH.track_prior_params(**bad)
    assert len(MH.REASONS) == 7


def test_the_frames_call_checks_before_any_launch():
    from metro_pose3d_amd import frames as FR
    import inspect
    sig = inspect.signature(FR.locate_tracked_poses_in_frames).parameters
    locate = inspect.signature(FR.locate_poses_in_frames).parameters
    assert all(k in sig for k in locate if k not in ('return_spread', 'return_uncertainty')), 'the rest of locate_poses_in_frames\' keywords'
    assert (sig['sigma_floor_mm'].default, sig['cov_scale'].default, sig['near_mm'].default, sig['depth'].default) == (30.0, 1.0, 100.0, 'none')
    follow = inspect.signature(FR.follow_poses_in_frames).parameters
    assert sig['max_age_s'].default == follow['max_age_s'].default and sig['accel_psd'].default == follow['accel_psd'].default
    assert FR.TrackedFramePoses._fields == ('plain', 'posterior', 'posterior_covariance', 'log_evidence', 'peak', 'reason')
    frame = np.zeros((64, 64, 3), np.uint8)
    with pytest.raises(ValueError, match='table_coords'):
        FR.locate_tracked_poses_in_frames(frame, np.zeros((1, 4)), 'none.npz', None, None, [0], None, [0.0], table_coords='crop')
    with pytest.raises(ValueError, match='sigma_floor_mm'):
        FR.locate_tracked_poses_in_frames(frame, np.zeros((1, 4)), 'none.npz', None, None, [0], None, [0.0], sigma_floor_mm=-1.0)
    with pytest.raises(ValueError, match='cameras'):
        FR.locate_tracked_poses_in_frames(frame, np.zeros((1, 4)), 'none.npz', None, None, [0], None, [0.0])
    follower = FR.Follower('none.npz', None, bone_lengths=np.ones(16))
    with pytest.raises(ValueError, match='call follow first'):
        follower.locate(frame, np.zeros((1, 4)), [0], None, [0.0])
    assert list(inspect.signature(FR.Follower.__init__).parameters) == ['self', 'model_path', 'cameras', 'world', 'assignment', 'capacity',
                                                                        'single_view', 'learn_bones', 'keywords']


# ---- the C surface ---------------------------------------------------------------------------------------------------------------

def test_symbol_in_header_bindings_and_library():
    header = open(os.path.join(ROOT, 'include', 'metro_hip.h')).read()
    proto = re.search(r'int\s+metro_plan_bind_track_prior\(([^;]*)\);', header).group(1)
    assert 'stream' not in proto, 'a bind entry takes no stream: no new launching entry'
    assert len(proto.split(',')) == len(_lib.SIGNATURES['metro_plan_bind_track_prior'][1]) == 13
    assert re.search(r'#define METRO_ABI_VERSION 8\b', header) and _lib.load().metro_abi_version() == 8
    assert C.sizeof(_lib.MetroTrackPrior) == 48
    for word in ('METRO_TRACK_PRIOR_DEPTH_NONE 0', 'METRO_TRACK_PRIOR_DEPTH_ROOT 1', 'correlation of z with the projected xy',
                 'correlation between a joint and its root'):
        assert word in header, word
    assert 'track_priors.hip' in open(os.path.join(ROOT, 'metro_pose3d_amd', 'build.py')).read()


def _plan(lib, spec, precision=1, max_batch=4):
    plan = C.c_void_p()
    cs = spec.to_c(precision)
    _lib.check(lib.metro_plan_create(C.byref(cs), max_batch, C.byref(plan)), 'metro_plan_create')
    return plan


def test_bind_refusals_without_a_device():
    """Every refusal of the bind entry returns METRO_ERR_INVALID_ARG; nothing is dereferenced at bind time, so fake (aligned)
    addresses stand for the device buffers."""
    lib = _lib.load()
    plan = _plan(lib, ModelSpec(50, 32, 'h36m', base_width=8))
    good = MH.track_prior_params('camera', 'root')
    ptrs = [C.c_void_p(4096 * (i + 1)) for i in range(9)]           # state, slot, times, records, mirror, prior, reason, post, scratch

    def bind(params=good, capacity=4, max_n=4, swap=None, pl=plan):
        p = list(ptrs)
        if swap is not None:
            p[swap[0]] = swap[1]
        return lib.metro_plan_bind_track_prior(pl, p[0], capacity, p[1], p[2], p[3], p[4], C.byref(params) if params is not None else None,
                                               p[5], p[6], p[7], p[8], max_n)
    try:
        assert bind() == 0
        assert lib.metro_plan_bind_prior(plan, ptrs[5], ptrs[7], ptrs[8], 4) == -1, 'bind_prior while a track table is bound'
        assert b'one prior per forward' in lib.metro_last_error()
        assert lib.metro_plan_bind_track_prior(plan, None, 0, None, None, None, None, None, None, None, None, None, 0) == 0
        assert lib.metro_plan_bind_prior(plan, ptrs[5], ptrs[7], ptrs[8], 4) == 0
        assert bind() == -1 and b'one prior per forward' in lib.metro_last_error(), 'and the reverse'
        assert lib.metro_plan_bind_prior(plan, None, None, None, 0) == 0
        for capacity in (0, 129, -1):
            assert bind(capacity=capacity) == -1 and b'capacity' in lib.metro_last_error()
        for max_n in (0, 5):
            assert bind(max_n=max_n) == -1
        for i in range(9):
            assert bind(swap=(i, None)) == -1, i
        assert bind(params=None) == -1
        assert bind(swap=(8, C.c_void_p(4096 * 9 + 8))) == -1 and bind(swap=(0, C.c_void_p(4100))) == -1, 'alignment'
        for field, value in (('coords', _lib.METRO_COORDS_CROP), ('coords', 7), ('depth', 2), ('accel_psd', -1.0), ('max_age_s', float('nan')),
                             ('near_mm', float('inf')), ('sigma_floor_mm', -0.5), ('cov_scale', float('nan'))):
            p = MH.track_prior_params('camera', 'root')
            setattr(p, field, value)
            assert bind(params=p) == -1, (field, value)
            assert field.encode() in lib.metro_last_error(), (field, lib.metro_last_error())
        assert bind() == 0 and bind(params=MH.track_prior_params('world', 'none'), capacity=128, max_n=1) == 0, 'rebinding'
        merged = _plan(lib, ModelSpec(50, 32, 'merged', base_width=8))
        try:
            assert bind(pl=merged) == -1 and b'root' in lib.metro_last_error(), 'DEPTH_ROOT without the root in the output order'
            assert bind(params=MH.track_prior_params('camera', 'none'), pl=merged) == 0
        finally:
            lib.metro_plan_destroy(merged)
    finally:
        lib.metro_plan_destroy(plan)


def test_forward_refusals_before_any_launch():
    """n > max_n, and a forward entry without a coords01 output while DEPTH_ROOT is bound: METRO_ERR_INVALID_ARG from the checks
    that run before the first launch (the plan has parameters bound to a fake blob; nothing is enqueued)."""
    lib = _lib.load()
    plan = _plan(lib, ModelSpec(50, 32, 'h36m', base_width=8), max_batch=4)
    ptrs = [C.c_void_p(4096 * (i + 1)) for i in range(9)]
    fake = C.c_void_p(1 << 20)
    try:
        assert lib.metro_plan_bind_params(plan, fake) == 0
        p = MH.track_prior_params('camera', 'root')
        assert lib.metro_plan_bind_track_prior(plan, ptrs[0], 4, ptrs[1], ptrs[2], ptrs[3], ptrs[4], C.byref(p), ptrs[5], ptrs[6], ptrs[7],
                                               ptrs[8], 2) == 0
        assert lib.metro_forward_coords01(plan, fake, 3, fake, fake, fake, None) == -1 and b'metro_plan_bind_track_prior' in lib.metro_last_error()
        assert lib.metro_forward(plan, fake, 2, fake, fake, None) == -1 and b'coords01' in lib.metro_last_error()
        assert lib.metro_forward_moments(plan, fake, 0, 2, fake, None, None, None, None, fake, None) == -1 and b'coords01' in lib.metro_last_error()
    finally:
        lib.metro_plan_destroy(plan)
