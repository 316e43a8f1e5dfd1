"""Per-joint heat-map covariance and peak on the MI355X: the MOMENTS instantiations of the head and soft-argmax kernels against
the fp64 restatement (tests/heat_moments_ref.py) of the kernel's OWN dumped fp32 logits -- which isolates the statistics from
the GEMM -- at the smallest shapes that reach every kernel variant, finalize branch and joint block; then Engine.forward,
estimate_pose and the frames chain.

Tolerances.  fp64 accumulators (precise 1 / 2): the standard deviations within 1e-3 mm, the bar the poses are held to.  fp32
accumulators (fused head, precise 0): the largest deviation of a Cov01 entry from the restatement, relative to
max(|entry scale|, the variance of one voxel (1 / (S - 1))^2 / 12), was measured over the cases below and recorded in
profiles/heat_moments_parity.json (tools/heat_moments_parity.py); the tests assert FOUR times that figure (other seeds, and the
fp32 fold order, which varies with the tile variant), and that the figure itself is below 1e-3: above it the accumulation
would not be centred."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from metro_pose3d_amd import ModelSpec, _lib
from metro_pose3d_amd._lib import check
from tests import helpers as H, heat_moments_ref as HM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = os.path.join(ROOT, 'profiles', 'heat_moments_parity.json')
DATASET = {17: 'h36m', 19: 'many19', 53: 'merged'}

# (id, c_in, stride (side = 256 / stride), n, J, expected kernel id): one row per code path of head_f16.hip
HEAD_CASES = [
    ('plain64', 320, 16, 1, 17, 'head_f16<160x64,moments>'),
    ('plain64-one-record', 320, 32, 2, 17, 'head_f16<160x64,moments>'),         # side 8: finalize folds ONE record per joint
    ('plain256', 320, 4, 16, 17, 'head_f16<160x256,moments>'),                  # wave-per-joint finalize (128 records)
    ('ring64', 2048, 16, 3, 17, 'head_f16<144x64,k4,moments>'),
    ('ring64-j19', 2048, 16, 3, 19, 'head_f16<160x64,k4,moments>'),             # J not a multiple of the 5-joint block
    ('ring64-groups', 2048, 16, 3, 53, 'head_f16<160x64,k4,g3,moments>'),       # joint-group form
    ('ring128', 2048, 4, 8, 17, 'head_f16<144x128,k4,moments>'),
    ('ring256', 2048, 4, 16, 17, 'head_f16<144x256,k2,moments>'),
]
GAINS = (1.0, 12.0)          # logit scales: a broad heat-map, and one a few voxels wide


def _noted(lib):
    return lib.metro_last_kernel_id().decode().split(' & ')


def _deviation(cov6_dev, cov_ref, side):
    """Largest |Cov01 entry - restatement| relative to max(sqrt(var_a var_b), the variance of one voxel)."""
    ref6 = HM.cov6(cov_ref)
    var = np.stack([cov_ref[..., a, a] for a in range(3)], -1)
    scale = np.stack([np.sqrt(var[..., a] * var[..., b]) for a, b in HM.COV6], -1)
    floor = (1.0 / (side - 1)) ** 2 / 12.0
    return float((np.abs(np.asarray(cov6_dev, np.float64) - ref6) / np.maximum(scale, floor)).max())


def _conditions(cov6, peak, what):
    cov6, peak = np.asarray(cov6, np.float64), np.asarray(peak, np.float64)
    assert np.isfinite(cov6).all() and np.isfinite(peak).all(), what
    assert (cov6[..., :3] >= 0).all(), (what, cov6[..., :3].min())
    for k, (a, b) in zip((3, 4, 5), ((0, 1), (0, 2), (1, 2))):
        assert (cov6[..., k] ** 2 <= cov6[..., a] * cov6[..., b] * (1 + 1e-6)).all(), (what, 'minor', a, b)
    assert (peak > 0).all() and (peak <= 1).all(), what


def run_head(lib, cuda, c_in, stride, n, nj, gain, seed=0):
    """One metro_head_f16_moments call on random weights -> dict of host arrays + the fp64 restatement of its dumped logits."""
    spec = ModelSpec(50, stride, DATASET[nj])
    side, c = spec.heatmap_side, spec.n_head_channels
    gen = torch.Generator(device=cuda).manual_seed(seed)
    rng = np.random.default_rng(seed)
    x = torch.randn((n, side, side, c_in), generator=gen, device=cuda, dtype=torch.float32).half()
    w = torch.from_numpy((rng.standard_normal((c, c_in)) * np.sqrt(2.0 / c_in) * gain).astype(np.float16)).to(cuda)
    b = torch.from_numpy((rng.standard_normal(c) * 0.1).astype(np.float32)).to(cuda)
    sc = torch.from_numpy(rng.uniform(0.5, 1.5, c_in).astype(np.float16)).to(cuda)
    sh = torch.from_numpy((rng.standard_normal(c_in) * 0.2).astype(np.float16)).to(cuda)
    cs = spec.to_c(_lib.METRO_PREC_F16)
    f32 = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=cuda)
    scratch = torch.empty(lib.metro_head_f16_scratch_bytes(n, side, nj), dtype=torch.uint8, device=cuda)
    mscratch = torch.empty(lib.metro_moments_scratch_bytes(C.byref(cs), n), dtype=torch.uint8, device=cuda)
    logits, poses, c01, cov, peak = f32(n, side, side, c), f32(n, spec.skeleton.n_out, 3), f32(n, nj, 3), f32(n, nj, 6), f32(n, nj)
    check(lib.metro_kernel_notes(1), 'notes')
    check(lib.metro_head_f16_moments(H.ptr(x), H.ptr(w), H.ptr(b), H.ptr(sc), H.ptr(sh), n, c_in, C.byref(cs), H.ptr(scratch),
                                     H.ptr(mscratch), H.ptr(logits), H.ptr(poses), H.ptr(c01), H.ptr(cov), H.ptr(peak), None),
          'metro_head_f16_moments')
    ids = _noted(lib)
    check(lib.metro_kernel_notes(0), 'notes')
    # the plain head on the same input, then coords01 of ITS finalize through the soft-argmax of nothing: poses only
    poses0 = f32(n, spec.skeleton.n_out, 3)
    scratch0 = torch.empty_like(scratch)
    check(lib.metro_head_f16(H.ptr(x), H.ptr(w), H.ptr(b), H.ptr(sc), H.ptr(sh), n, c_in, C.byref(cs), H.ptr(scratch0), None,
                             H.ptr(poses0), None), 'metro_head_f16')
    torch.cuda.synchronize()
    mu, cov_ref, peak_ref, _ = HM.moments(logits.cpu().numpy(), nj, spec.depth)
    records = n * (side * side // (64 if ids[0].startswith('head_f16<160x64') and ',k' not in ids[0] else 32)) * nj * 5
    return dict(spec=spec, ids=ids, poses=poses, poses0=poses0, rec=scratch.view(torch.float32)[:records],
                rec0=scratch0.view(torch.float32)[:records], c01=c01.cpu().numpy(), cov=cov.cpu().numpy(),
                peak=peak.cpu().numpy(), mu=mu, cov_ref=cov_ref, peak_ref=peak_ref)


def run_softargmax(lib, cuda, spec, logits, precise):
    """metro_softargmax01_moments and metro_softargmax01 on the same logits -> (c01, cov6, peak, c01 of the plain entry)."""
    n, nj = logits.shape[0], spec.skeleton.n_head
    cs = spec.to_c(int(precise))
    tl = torch.from_numpy(np.ascontiguousarray(logits.astype(np.float64 if precise == 2 else np.float32))).to(cuda)
    scratch = torch.empty(lib.metro_softargmax_scratch_bytes(n, spec.heatmap_side, nj), dtype=torch.uint8, device=cuda)
    mscratch = torch.empty(lib.metro_moments_scratch_bytes(C.byref(cs), n), dtype=torch.uint8, device=cuda)
    f32 = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=cuda)
    c01, cov, peak, c01_plain = f32(n, nj, 3), f32(n, nj, 6), f32(n, nj), f32(n, nj, 3)
    check(lib.metro_softargmax01_moments(H.ptr(tl), n, C.byref(cs), precise, H.ptr(scratch), H.ptr(mscratch), H.ptr(c01), H.ptr(cov),
                                         H.ptr(peak), None), 'metro_softargmax01_moments')
    check(lib.metro_softargmax01(H.ptr(tl), n, C.byref(cs), precise, H.ptr(scratch), H.ptr(c01_plain), None), 'metro_softargmax01')
    torch.cuda.synchronize()
    return c01, cov.cpu().numpy(), peak.cpu().numpy(), c01_plain


def random_logits(spec, n, gain, seed):
    rng = np.random.default_rng([seed, spec.heatmap_side, spec.depth])
    return (rng.standard_normal((n, spec.heatmap_side, spec.heatmap_side, spec.n_head_channels)) * gain).astype(np.float32)


SA_SPECS = {'side16': (ModelSpec(50, 16, 'h36m'), 2), 'side16-d4': (ModelSpec(50, 16, 'h36m', depth=4), 2),
            'side8': (ModelSpec(50, 32, 'h36m'), 2), 'side64': (ModelSpec(50, 4, 'h36m'), 1)}


def fp32_deviations(lib, cuda):
    """Every fp32-accumulator case of this file -> {case: deviation}: what tools/heat_moments_parity.py records."""
    out = {}
    for name, c_in, stride, n, nj, _ in HEAD_CASES:
        for gain in GAINS:
            r = run_head(lib, cuda, c_in, stride, n, nj, gain)
            out[f'head/{name}/gain{gain:g}'] = _deviation(r['cov'], r['cov_ref'], r['spec'].heatmap_side)
    for name, (spec, n) in SA_SPECS.items():
        for gain in (1.0, 8.0):
            lg = random_logits(spec, n, gain, 1)
            _, cov, _, _ = run_softargmax(lib, cuda, spec, lg, 0)
            out[f'softargmax0/{name}/gain{gain:g}'] = _deviation(cov, HM.moments(lg, spec.skeleton.n_head, spec.depth)[1], spec.heatmap_side)
    return out


def _fp32_bound():
    rec = json.load(open(PARITY))
    measured = float(rec['max_relative_deviation'])
    assert 0 < measured <= 1e-3, f'recorded deviation {measured}: the accumulation is not centred'
    return 4.0 * measured


@pytest.mark.parametrize('gain', GAINS, ids=lambda g: f'gain{g:g}')
@pytest.mark.parametrize('case', HEAD_CASES, ids=lambda c: c[0])
def test_head_moments_match_the_restatement_of_the_dumped_logits(lib, cuda, case, gain):
    name, c_in, stride, n, nj, kid = case
    r = run_head(lib, cuda, c_in, stride, n, nj, gain)
    assert r['ids'] == [kid, 'softargmax_finalize<acc32,moments>'], r['ids']
    assert torch.equal(r['rec'], r['rec0']), 'the 5-word records differ from the plain head kernel'
    assert torch.equal(r['poses'], r['poses0']), 'poses differ from the plain head'
    _conditions(r['cov'], r['peak'], name)
    dev = _deviation(r['cov'], r['cov_ref'], r['spec'].heatmap_side)
    print(f'{name} gain {gain:g}: Cov01 deviation {dev:.3e}, largest sd01 {np.sqrt(r["cov_ref"].max()):.3f}, peak {r["peak_ref"].min():.2e} .. {r["peak_ref"].max():.2e}')
    assert dev <= _fp32_bound(), (name, gain, dev)
    # __expf: v_exp_f32(x log2 e), the product rounds at |x| ulp, |x| < 17 for every term above an fp32 ulp of the sum
    assert np.allclose(r['peak'], r['peak_ref'], rtol=1e-5, atol=0)
    assert np.abs(r['c01'] - r['mu']).max() <= 2e-6


def test_head_coords01_equal_the_plain_forward_path(lib, cuda):
    """coords01 next to the moments are the bits of the plain finalize on the same records (metro_softargmax01 has no head
    form: the plain launch_softargmax_finalize is reached through metro_head_f16's poses, compared above; here through the
    logits dump and the two-launch soft-argmax, within its fp32 rounding)."""
    r = run_head(lib, cuda, 2048, 16, 3, 17, 12.0, seed=3)
    assert np.abs(r['c01'] - r['mu']).max() <= 2e-6


@pytest.mark.parametrize('precise', [0, 1, 2])
@pytest.mark.parametrize('name', sorted(SA_SPECS))
def test_softargmax_moments_match_the_restatement(lib, cuda, name, precise):
    spec, n = SA_SPECS[name]
    nj, side = spec.skeleton.n_head, spec.heatmap_side
    for gain in (1.0, 8.0):
        lg = random_logits(spec, n, gain, 1)
        c01, cov, peak, c01_plain = run_softargmax(lib, cuda, spec, lg, precise)
        assert torch.equal(c01, c01_plain), 'coords01 differ from metro_softargmax01'
        _conditions(cov, peak, name)
        mu, cov_ref, peak_ref, _ = HM.moments(lg, nj, spec.depth)
        dev = _deviation(cov, cov_ref, side)
        s = HM.metric_scale(spec)
        sd_dev = np.sqrt(np.maximum(cov[..., :3], 0)) * s
        sd_ref = np.sqrt(np.stack([cov_ref[..., a, a] for a in range(3)], -1)) * s
        print(f'{name} precise {precise} gain {gain:g}: Cov01 deviation {dev:.3e}, sd deviation {np.abs(sd_dev - sd_ref).max():.3e} mm')
        if precise == 0:
            assert dev <= _fp32_bound(), (name, gain, dev)
            assert np.allclose(peak, peak_ref, rtol=1e-5, atol=0)
        else:
            assert np.abs(sd_dev - sd_ref).max() <= 1e-3, (name, gain)
            # cross terms on the same bar: 1e-3 mm against the standard deviations they sit between
            cross = cov[..., 3:] * np.array([s[0] * s[1], s[0] * s[2], s[1] * s[2]])
            cross_ref = HM.cov6(cov_ref)[..., 3:] * np.array([s[0] * s[1], s[0] * s[2], s[1] * s[2]])
            assert (np.abs(cross - cross_ref) <= 1e-3 * np.maximum(sd_ref[..., [0, 0, 1]], sd_ref[..., [1, 2, 2]]) + 1e-6).all()
            assert np.allclose(peak, peak_ref, rtol=2e-7, atol=0)


@pytest.mark.parametrize('precise', [0, 1, 2])
def test_crafted_volumes(lib, cuda, precise):
    """One-hot (variance exactly 0, peak 1), uniform (the variance of a linspace, no cross terms) and a peak in the corner voxel of
    the last slab next to a broad background."""
    spec = ModelSpec(50, 16, 'h36m')
    nj, side, depth = spec.skeleton.n_head, spec.heatmap_side, spec.depth
    lg = np.zeros((3, side, side, depth * nj), np.float32)
    hot = np.random.default_rng(7).integers(0, [side, side, depth], (nj, 3))
    hot[0], hot[1] = (0, 0, 0), (side - 1, side - 1, depth - 1)
    lg[0] = -1e4
    for j, (y, x, d) in enumerate(hot):
        lg[0, y, x, d * nj + j] = 0.0
    lg[2] = np.random.default_rng(8).standard_normal(lg[2].shape)
    lg[2, side - 1, side - 1, (depth - 1) * nj:] = 9.0               # every joint: the last voxel of the last slab
    c01, cov, peak, c01_plain = run_softargmax(lib, cuda, spec, lg, precise)
    assert torch.equal(c01, c01_plain)
    _conditions(cov, peak, 'crafted')
    assert (cov[0] == 0).all() and (peak[0] == 1).all(), (cov[0].max(), peak[0].min())
    want = c01.cpu().numpy()[0]
    assert np.array_equal(want, np.stack([HM.lin01(side)[hot[:, 1]], HM.lin01(side)[hot[:, 0]], HM.lin01(depth)[hot[:, 2]]], -1).astype(np.float32))
    var = lambda k: (k + 1) / (12.0 * (k - 1))
    tol = 1e-6 if precise else _fp32_bound()
    assert np.allclose(cov[1][:, :3], [var(side), var(side), var(depth)], rtol=tol, atol=0)
    assert np.abs(cov[1][:, 3:]).max() <= tol * var(depth)
    assert np.allclose(peak[1], 1.0 / (side * side * depth), rtol=1e-6)
    cov_ref, peak_ref = HM.moments(lg[2:], nj, depth)[1:3]
    assert _deviation(cov[2:], cov_ref, side) <= (1e-6 if precise else _fp32_bound())
    assert np.allclose(peak[2:], peak_ref, rtol=1e-5)


def test_recorded_parity_figure_covers_these_cases():
    rec = json.load(open(PARITY))
    names = {f'head/{c[0]}/gain{g:g}' for c in HEAD_CASES for g in GAINS} | \
            {f'softargmax0/{k}/gain{g:g}' for k in SA_SPECS for g in (1.0, 8.0)}
    assert set(rec['cases']) == names
    assert rec['max_relative_deviation'] == max(rec['cases'].values())


# ---- end to end ------------------------------------------------------------------------------------------------------------

def _engine_case(stride, base_width, seed=1):
    from metro_pose3d_amd import synth
    spec = ModelSpec(50, stride, 'h36m', base_width=base_width)
    params = synth.make_params(50, spec.n_head_channels, base_width, seed=seed, logit_gain=synth.logit_gain_for(50, stride, base_width))
    return spec, params


def _forward_with_moments(eng, x):
    n, sk = x.shape[0], eng.spec.skeleton
    f32 = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=x.device)
    c01, cov, peak = f32(n, sk.n_head, 3), f32(n, sk.n_head, 6), f32(n, sk.n_head)
    poses = eng.forward(x, coords01=c01, cov01=cov, peak=peak)
    return poses, c01, cov, peak


# the narrow nets (base width 8: 256 head input channels, the 64-pixel head) in every precision, the full-width net (2048
# channels: the ring head) in f16
@pytest.mark.parametrize('stride,base_width,precision', [(16, 8, 'f16'), (32, 8, 'f16'), (16, 8, 'f32m'), (32, 8, 'f32m'),
                                                         (16, 8, 'f64'), (32, 8, 'f64'), (16, 64, 'f16'), (32, 64, 'f16')])
def test_engine_forward_moments(cuda, stride, base_width, precision):
    from metro_pose3d_amd import synth
    from metro_pose3d_amd.engine import Engine
    spec, params = _engine_case(stride, base_width)
    eng = Engine(spec, params, precision, max_batch=4, device=cuda)
    sk = spec.skeleton
    imgs = synth.make_images(3, spec.proc_side, seed=5)
    x = torch.from_numpy(imgs).to(cuda)
    xb = torch.from_numpy(np.round(imgs * 255).astype(np.uint8)).to(cuda)
    for inp in (x, xb):
        c01_plain = torch.empty((3, sk.n_head, 3), device=cuda)
        poses_plain = eng.forward(inp, coords01=c01_plain).clone()
        poses, c01, cov, peak = _forward_with_moments(eng, inp)
        assert torch.equal(poses, poses_plain) and torch.equal(c01, c01_plain), (precision, inp.dtype)
        assert torch.equal(eng.forward(inp), poses_plain)
        _conditions(cov.cpu().numpy(), peak.cpu().numpy(), precision)
        logits = eng.forward_upto(inp, len(eng.layer_infos()) - 2).cpu().numpy()
        mu, cov_ref, peak_ref, _ = HM.moments(logits, sk.n_head, spec.depth)
        dev = _deviation(cov.cpu().numpy(), cov_ref, spec.heatmap_side)
        print(f'stride {stride} width {base_width} {precision} {inp.dtype}: Cov01 deviation {dev:.3e}')
        if precision == 'f16':
            assert dev <= _fp32_bound()
        else:
            s = HM.metric_scale(spec)
            sd = np.sqrt(np.maximum(cov.cpu().numpy()[..., :3], 0)) * s
            sd_ref = np.sqrt(np.stack([cov_ref[..., a, a] for a in range(3)], -1)) * s
            assert np.abs(sd - sd_ref).max() <= 1e-3
        assert np.allclose(peak.cpu().numpy(), peak_ref, rtol=1e-5)
    eng.close()


@pytest.mark.parametrize('precision', ['f16', 'f64'])
def test_estimate_pose_returns_the_uncertainty_in_output_order(cuda, tmp_path, precision):
    from metro_pose3d_amd import inference as INF, save_model, synth
    from metro_pose3d_amd.engine import Engine
    spec, params = _engine_case(32, 8)
    path = str(tmp_path / 'm.npz')
    save_model(path, spec, params)
    x = torch.from_numpy(synth.make_images(3, spec.proc_side, seed=6)).to(cuda)
    poses, edges, names, unc = INF.estimate_pose(x, path, precision=precision, return_uncertainty=True)
    plain = INF.estimate_pose(x, path, precision=precision)
    assert len(plain) == 3 and torch.equal(plain[0], poses)
    eng = Engine(spec, params, precision, max_batch=8, device=cuda)
    _, _, cov, peak = _forward_with_moments(eng, x)
    perm = np.asarray(spec.skeleton.permutation)
    s = HM.metric_scale(spec)
    c6 = cov.cpu().numpy().astype(np.float64)[:, perm]
    want = np.empty(c6.shape[:2] + (3, 3))
    for k, (a, b) in enumerate(HM.COV6):
        want[..., a, b] = want[..., b, a] = c6[..., k] * s[a] * s[b]
    assert unc.covariance.shape == (3, spec.skeleton.n_out, 3, 3) and unc.peak.shape == (3, spec.skeleton.n_out)
    assert np.allclose(unc.covariance.cpu().numpy(), want, rtol=1e-6, atol=0)
    assert torch.equal(unc.peak, peak[:, torch.from_numpy(perm).to(cuda)])
    eng.close()
    INF.clear_cache()


# ---- frames ----------------------------------------------------------------------------------------------------------------

def _frames_scene():
    from metro_pose3d_amd.frames import Camera
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 256, (120, 160, 3), dtype=np.uint8), rng.integers(0, 256, (100, 140, 3), dtype=np.uint8)]
    ang = 0.3
    rot = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    cam = Camera(np.array([[150.0, 0, 80], [0, 150.0, 60], [0, 0, 1]]), np.array([-0.2, 0.05, 0.001, -0.002, 0.01], np.float32),
                 R=rot, t=np.array([100.0, -50.0, 30.0]), world_up=(0, -1, 0))
    boxes = np.array([[20.0, 10, 60, 90], [70, 30, 50, 60], [30, 20, 70, 70]])
    return frames, cam, boxes, np.array([0, 0, 1])


@pytest.mark.parametrize('device_boxes', [False, True], ids=['host-boxes', 'cuda-boxes'])
@pytest.mark.parametrize('views', [None, [(-15, 1.0, False), (0, 1.1, True), (10, 1.0, False)]], ids=['one-view', 'three-views'])
def test_frames_covariance_is_rotated_mirrored_and_averaged(cuda, tmp_path, views, device_boxes):
    from metro_pose3d_amd import frames as FR, inference as INF, save_model
    spec, params = _engine_case(32, 8)
    path = str(tmp_path / 'm.npz')
    save_model(path, spec, params)
    sk = spec.skeleton
    frames, cam, boxes, fi = _frames_scene()
    vs = FR.view_set(1 if views is None else views)
    nv, n = len(vs.zoom), len(boxes)
    # the per-view engine output, through the chain's own warp
    eng = INF._engine_for(path, 'f16', cuda, n * nv)
    with torch.cuda.device(cuda):
        crops, places = FR._warp_views(FR._frame_set(frames, 'rgb', 'bt601'), cam, boxes, fi, vs, spec.proc_side, cuda)
    _, _, cov, peak = _forward_with_moments(eng, crops)
    rec = np.ascontiguousarray(places.cpu().numpy()).view(np.dtype(_lib.MetroPlacement)).ravel()
    perm, mirror, s = np.asarray(sk.permutation), np.asarray(sk.out_mirror), HM.metric_scale(spec)
    c6 = cov.cpu().numpy().astype(np.float64)
    full = np.empty(c6.shape[:2] + (3, 3))
    for k, (a, b) in enumerate(HM.COV6):
        full[..., a, b] = full[..., b, a] = c6[..., k] * s[a] * s[b]
    pk = peak.cpu().numpy().astype(np.float64)
    bx = torch.from_numpy(boxes).to(cuda) if device_boxes else boxes
    fidx = torch.from_numpy(fi.astype(np.int32)).to(cuda) if device_boxes else fi
    for coords in ('crop', 'camera', 'world') if nv == 1 else ('camera', 'world'):
        want, want_pk = np.zeros((n, sk.n_out, 3, 3)), np.zeros((n, sk.n_out))
        flipped = 0
        for i in range(n):
            for v in range(nv):
                row = i * nv + v
                R = np.eye(3) if coords == 'crop' else rec['rot_to_orig_cam' if coords == 'camera' else 'rot_to_world'][row].reshape(3, 3).astype(np.float64)
                mir = coords != 'crop' and not np.linalg.det(R) > 0
                flipped += mir
                src = perm[mirror] if mir else perm
                rotated = R @ full[row, src] @ R.T
                assert np.allclose(np.linalg.eigvalsh(rotated), np.linalg.eigvalsh(full[row, src]), rtol=1e-5, atol=0)
                want[i] += rotated / nv
                want_pk[i] += pk[row, src] / nv
        assert flipped == (n if nv == 3 else 0)
        res = FR.estimate_pose_in_frames(frames, bx, path, cameras=cam, frame_index=fidx, coords=coords, views=views,
                                         return_uncertainty=True)
        plain = FR.estimate_pose_in_frames(frames, bx, path, cameras=cam, frame_index=fidx, coords=coords, views=views)
        assert len(plain) == 3 and torch.equal(plain[0], res[0])
        got, got_pk = res[3].covariance.cpu().numpy(), res[3].peak.cpu().numpy()
        if not device_boxes:       # device geometry: records within a few fp32 ulp of the host's, not its bits
            assert np.allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(want).max()), coords
            assert np.allclose(got_pk, want_pk, rtol=1e-6)
        else:
            assert np.allclose(got, want, rtol=1e-3, atol=1e-3 * np.abs(want).max()), coords
            assert np.allclose(got_pk, want_pk, rtol=1e-3)
        assert np.allclose(got, np.swapaxes(got, -1, -2)) and (np.linalg.eigvalsh(got.astype(np.float64)) > -1e-3).all()
        loc = FR.locate_poses_in_frames(frames, bx, path, cameras=cam, frame_index=fidx, coords=coords, views=views,
                                        scale_recovery='metro', return_uncertainty=True)
        assert torch.equal(loc.covariance, res[3].covariance) and torch.equal(loc.peak, res[3].peak)
        assert FR.locate_poses_in_frames(frames, bx, path, cameras=cam, frame_index=fidx, coords=coords, views=views,
                                         scale_recovery='metro').covariance is None
    # uint8 crops and another pixel format go through the same launches
    res8 = FR.estimate_pose_in_frames(frames, bx, path, cameras=cam, frame_index=fidx, views=views, crop_dtype='uint8',
                                      return_uncertainty=True)
    ref = FR.estimate_pose_in_frames(frames, bx, path, cameras=cam, frame_index=fidx, views=views, return_uncertainty=True)
    assert torch.equal(res8[3].covariance, ref[3].covariance) and torch.equal(res8[3].peak, ref[3].peak)
    bgr = [f[..., ::-1].copy() for f in frames]
    resb = FR.estimate_pose_in_frames(bgr, bx, path, cameras=cam, frame_index=fidx, views=views, pixel_format='bgr',
                                      return_uncertainty=True)
    assert torch.equal(resb[3].covariance, ref[3].covariance)
    INF.clear_cache()
