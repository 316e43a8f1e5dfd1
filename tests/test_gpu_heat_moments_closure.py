"""The MOMENTS instantiations of the head and soft-argmax kernels on the MI355X at the points tests/test_heat_moments_closure.py
derives from the dispatch (`-m gpu`): every moments id of the supported grid, every (id, head side, joints, depth) of
proc_side 256, each id's smallest side that is not a power of two and its largest; the two-launch soft-argmax at ragged sides
and every head; metro_forward_moments where the plan picks the 128- and 256-pixel-tile heads; and non-finite inputs through
each of the five kernels.

The references and the bars are those of tests/test_gpu_heat_moments.py (the fp64 restatement of the kernel's OWN dumped logits;
four times the recorded fp32 figure of profiles/heat_moments_parity.json, which these cases do not enter).  The head batches
are laid out as in tests/test_kernel_coverage.py: min(4, n) base images at positions drawn by helpers.crop_assignment, the
restatement on the base images, every other position holding its twin's bits -- a record stored into another image's slot
fails the twin check."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from metro_pose3d_amd import ModelSpec, _lib
from metro_pose3d_amd._lib import check
from tests import helpers as H, heat_moments_ref as HM
from tests.test_gpu_heat_moments import (_conditions, _deviation, _fp32_bound, _forward_with_moments, _noted, random_logits,
                                         run_softargmax)
from tests.test_heat_moments_closure import HEAD_CLOSURE_CASES, SA_CLOSURE_CASES, with_moments
from tests.test_kernel_coverage import spec_name

pytestmark = pytest.mark.gpu

GAINS = (1.0, 12.0)             # logit scales: a broad heat-map, and one a few voxels wide
FIN = 'softargmax_finalize<acc32,moments>'
BASE_IMAGES = 4


def _bits(t):
    return t.contiguous().view(torch.int32)


def _moments_by_image(logits, nj, depth):
    """HM.moments an image at a time (a 128 x 128 map of 53 joints is 7 M voxels: the restatement's temporaries stay small)."""
    parts = [HM.moments(logits[i:i + 1], nj, depth)[:3] for i in range(logits.shape[0])]
    return [np.concatenate([p[k] for p in parts]) for k in range(3)]


def _head_operands(spec, n, c_in, gain, what, cuda):
    """The operands of run_head (tests/test_gpu_heat_moments.py) with the batch of test_kernel_coverage._head: base images laid
    out as twins, seeded by the case."""
    seed = zlib.crc32(what.encode())
    side, c = spec.heatmap_side, spec.n_head_channels
    gen = torch.Generator(device=cuda).manual_seed(seed)
    rng = np.random.default_rng(seed)
    p = min(BASE_IMAGES, n)
    assign = H.crop_assignment(n, p, seed)
    base = torch.randn((p, side, side, c_in), generator=gen, device=cuda, dtype=torch.float32).half()
    x = H.lay_out_twins(base, assign)
    del base
    w = torch.from_numpy((rng.standard_normal((c, c_in)) * np.sqrt(2.0 / c_in) * gain).astype(np.float16)).to(cuda)
    b = torch.from_numpy((rng.standard_normal(c) * 0.1).astype(np.float32)).to(cuda)
    sc = torch.from_numpy(rng.uniform(0.5, 1.5, c_in).astype(np.float16)).to(cuda)
    sh = torch.from_numpy((rng.standard_normal(c_in) * 0.2).astype(np.float16)).to(cuda)
    return assign, p, x, (w, b, sc, sh)


def launch_head(lib, cuda, spec, n, c_in, x, params, moments=True, logits=True):
    """One metro_head_f16_moments (or metro_head_f16) call, outputs filled with NaN first -> dict of device tensors + noted ids."""
    side, c, nj = spec.heatmap_side, spec.n_head_channels, spec.skeleton.n_head
    w, b, sc, sh = params
    cs = spec.to_c(_lib.METRO_PREC_F16)
    f32 = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=cuda)
    nbytes = lib.metro_head_f16_scratch_bytes(n, side, nj)
    r = dict(scratch=torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=cuda), poses=f32(n, spec.skeleton.n_out, 3),
             logits=f32(n, side, side, c) if logits else None)
    check(lib.metro_kernel_notes(1), 'notes')
    try:
        if moments:
            r['mscratch'] = torch.full((lib.metro_moments_scratch_bytes(C.byref(cs), n),), 0xFF, dtype=torch.uint8, device=cuda)
            r.update(c01=f32(n, nj, 3), cov=f32(n, nj, 6), peak=f32(n, nj))
            check(lib.metro_head_f16_moments(H.ptr(x), H.ptr(w), H.ptr(b), H.ptr(sc), H.ptr(sh), n, c_in, C.byref(cs), H.ptr(r['scratch']),
                                             H.ptr(r['mscratch']), H.ptr(r['logits']), H.ptr(r['poses']), H.ptr(r['c01']), H.ptr(r['cov']),
                                             H.ptr(r['peak']), None), 'metro_head_f16_moments')
        else:
            check(lib.metro_head_f16(H.ptr(x), H.ptr(w), H.ptr(b), H.ptr(sc), H.ptr(sh), n, c_in, C.byref(cs), H.ptr(r['scratch']),
                                     H.ptr(r['logits']), H.ptr(r['poses']), None), 'metro_head_f16')
        torch.cuda.synchronize()
        r['ids'] = _noted(lib)
    finally:
        lib.metro_kernel_notes(0)
    per = 64 if r['ids'][0].startswith('head_f16<160x64') and ',k' not in r['ids'][0] else 32      # pixels per 5-word record
    r['rec'] = r['scratch'].view(torch.float32)[:n * (side * side // per) * nj * 5]
    return r


# ---- 2. one metro_head_f16_moments launch per point of the closure ----------------------------------------------------------
@pytest.mark.parametrize('gain', GAINS, ids=lambda g: f'gain{g:g}')
@pytest.mark.parametrize('spec,n,ids', HEAD_CLOSURE_CASES)
def test_head_moments_closure(lib, cuda, spec, n, ids, gain):
    """Full-width head input (K = 2048).  The moments launch notes the ids the dry run named; its 5-word records, poses and fp32
    logits dump are the plain head's bits (include/metro_hip.h: 'same launch count; poses, coords01 ... have the bits of those
    entries'); every position carries its twin's bits; the base images match the fp64 restatement of their own dumped logits
    under the bars of test_head_moments_match_the_restatement_of_the_dumped_logits.

    Gain 12: the map is a few voxels wide and the means lie anywhere in the volume, so the comparison is not one of map centres
    -- asserted as max |mu - 0.5| > 0.25 (the logits are ~N(0, 12^2) over >= 512 voxels per joint: the largest few carry the
    mass, and their place is uniform over the volume; 0.498 for the 16 x 16, 17-joint head).  At gain 1 (0.124 there) the
    maps are broad and it is not asserted."""
    assert spec is not None, f'libmetro_hip.so could not be loaded at collection time: {ids}'
    what = f'{spec_name(spec)}-b{n}/{ids}'
    nj, side = spec.skeleton.n_head, spec.heatmap_side
    assign, p, x, params = _head_operands(spec, n, 2048, gain, what, cuda)
    r = launch_head(lib, cuda, spec, n, 2048, x, params)
    assert ' & '.join(r['ids']) == ids and r['ids'][1] == FIN, (r['ids'], ids)
    r0 = launch_head(lib, cuda, spec, n, 2048, x, params, moments=False)
    assert with_moments(' & '.join(r0['ids'])) == ids, r0['ids']
    assert torch.equal(_bits(r['rec']), _bits(r0['rec'])), 'the 5-word records differ from the plain head kernel'
    assert torch.equal(_bits(r['poses']), _bits(r0['poses'])), 'poses differ from the plain head'
    assert torch.equal(_bits(r['logits']), _bits(r0['logits'])), 'the fp32 logits dump differs from the plain head'
    del r0
    for name in ('cov', 'peak', 'c01', 'poses', 'logits'):
        H.assert_twins(r[name], assign, p, f'{ids} ({name})')
    cov, peak, c01 = (r[k][:p].cpu().numpy() for k in ('cov', 'peak', 'c01'))
    mu, cov_ref, peak_ref = _moments_by_image(r['logits'][:p].cpu().numpy(), nj, spec.depth)
    _conditions(cov, peak, what)
    dev = _deviation(cov, cov_ref, side)
    print(f'\n[{ids.split(" & ")[0]}] side {side}, {nj} joints, {n} crops, gain {gain:g}: Cov01 deviation {dev:.3e} (bar {_fp32_bound():.3e}), '
          f'largest sd01 {np.sqrt(cov_ref.max()):.3f}, peak {peak_ref.min():.2e} .. {peak_ref.max():.2e}, max |mu - 0.5| {np.abs(mu - 0.5).max():.3f}')
    assert dev <= _fp32_bound(), (what, gain, dev)
    assert np.allclose(peak, peak_ref, rtol=1e-5, atol=0)
    assert np.abs(c01 - mu).max() <= 2e-6
    if gain == 12.0:
        assert np.abs(mu - 0.5).max() > 0.25, np.abs(mu - 0.5).max()


# ---- 3. the two-launch soft-argmax with moments at ragged sides and every head ------------------------------------------------
def _crafted(spec):
    """test_crafted_volumes' three volumes at this head: one-hot per joint (joint 0 the first voxel, joint 1 the last voxel of the
    last slab), uniform, and a broad background with every joint's peak in the last voxel of the last slab."""
    nj, side, depth = spec.skeleton.n_head, spec.heatmap_side, spec.depth
    seed = [side, nj]
    lg = np.zeros((3, side, side, depth * nj), np.float32)
    hot = np.random.default_rng(seed + [7]).integers(0, [side, side, depth], (nj, 3))
    hot[0], hot[1] = (0, 0, 0), (side - 1, side - 1, depth - 1)
    lg[0] = -1e4
    for j, (y, x, d) in enumerate(hot):
        lg[0, y, x, d * nj + j] = 0.0
    lg[2] = np.random.default_rng(seed + [8]).standard_normal(lg[2].shape)
    lg[2, side - 1, side - 1, (depth - 1) * nj:] = 9.0
    return lg, hot


@pytest.mark.parametrize('precise', [0, 1, 2])
@pytest.mark.parametrize('spec,n', SA_CLOSURE_CASES)
def test_softargmax_moments_closure(lib, cuda, spec, n, precise):
    """metro_softargmax01_moments against the restatement under the bars of test_softargmax_moments_match_the_restatement and
    test_crafted_volumes, coords01 the bits of metro_softargmax01 on the same logits, the ids those the entry names."""
    assert spec is not None, 'libmetro_hip.so could not be loaded at collection time'
    nj, side, depth = spec.skeleton.n_head, spec.heatmap_side, spec.depth
    name = f'side {side}, {nj} joints, precise {precise}'
    acc, lgt = (32, 32) if precise == 0 else (64, 32) if precise == 1 else (64, 64)
    want_ids = [f'softargmax_partial<acc{acc},logits{lgt},moments>', f'softargmax_finalize<acc{acc},moments>']
    s = HM.metric_scale(spec)
    cross_s = np.array([s[0] * s[1], s[0] * s[2], s[1] * s[2]])
    for gain in (1.0, 8.0):
        lg = random_logits(spec, n, gain, 1)
        check(lib.metro_kernel_notes(1), 'notes')
        try:
            c01, cov, peak, c01_plain = run_softargmax(lib, cuda, spec, lg, precise)
            ids = _noted(lib)
        finally:
            lib.metro_kernel_notes(0)
        assert ids == want_ids + [k.replace(',moments', '') for k in want_ids], ids
        assert torch.equal(_bits(c01), _bits(c01_plain)), 'coords01 differ from metro_softargmax01'
        _conditions(cov, peak, name)
        mu, cov_ref, peak_ref, _ = HM.moments(lg, nj, depth)
        assert np.isfinite(cov_ref).all() and np.isfinite(peak_ref).all()
        dev = _deviation(cov, cov_ref, side)
        sd_dev = np.sqrt(np.maximum(cov[..., :3], 0)) * s
        sd_ref = np.sqrt(np.stack([cov_ref[..., a, a] for a in range(3)], -1)) * s
        print(f'\n[{want_ids[0]}] {name}, gain {gain:g}: Cov01 deviation {dev:.3e}, sd deviation {np.abs(sd_dev - sd_ref).max():.3e} mm')
        if precise == 0:
            assert dev <= _fp32_bound(), (name, gain, dev)
            assert np.allclose(peak, peak_ref, rtol=1e-5, atol=0)
        else:
            assert np.abs(sd_dev - sd_ref).max() <= 1e-3, (name, gain)
            cross, cross_ref = cov[..., 3:] * cross_s, HM.cov6(cov_ref)[..., 3:] * cross_s
            assert (np.abs(cross - cross_ref) <= 1e-3 * np.maximum(sd_ref[..., [0, 0, 1]], sd_ref[..., [1, 2, 2]]) + 1e-6).all()
            assert np.allclose(peak, peak_ref, rtol=2e-7, atol=0)
    lg, hot = _crafted(spec)
    c01, cov, peak, c01_plain = run_softargmax(lib, cuda, spec, lg, precise)
    assert torch.equal(_bits(c01), _bits(c01_plain))
    _conditions(cov, peak, name + ' (crafted)')
    assert (cov[0] == 0).all() and (peak[0] == 1).all(), (cov[0].max(), peak[0].min())
    want = np.stack([HM.lin01(side)[hot[:, 1]], HM.lin01(side)[hot[:, 0]], HM.lin01(depth)[hot[:, 2]]], -1).astype(np.float32)
    assert np.array_equal(c01.cpu().numpy()[0], want)
    var = lambda k: (k + 1) / (12.0 * (k - 1))               # the variance of linspace(0, 1, k) under equal weights
    tol = 1e-6 if precise else _fp32_bound()
    assert np.allclose(cov[1][:, :3], [var(side), var(side), var(depth)], rtol=tol, atol=0), name
    assert np.abs(cov[1][:, 3:]).max() <= tol * var(depth), name
    assert np.allclose(peak[1], 1.0 / (side * side * depth), rtol=1e-6)
    cov_ref, peak_ref = HM.moments(lg[2:], nj, depth)[1:3]
    assert _deviation(cov[2:], cov_ref, side) <= tol, name
    assert np.allclose(peak[2:], peak_ref, rtol=1e-5)


# ---- 4. metro_forward_moments where the plan picks the wide-tile heads -------------------------------------------------------
FORWARD_CASES = [
    # RN50-s4 h36m at 16 crops (BASELINE's C5 shape), RN50-s8 many19 at 32 crops
    pytest.param(4, 'h36m', 16, 'head_f16<144x256,k2>', id='rn50-s4-h36m-b16'),
    pytest.param(8, 'many19', 32, 'head_f16<160x128,k4>', id='rn50-s8-many19-b32'),
]


def _full_width_engine(cuda, stride, dataset, n, seed=1):
    from metro_pose3d_amd import synth
    from metro_pose3d_amd.engine import Engine
    spec = ModelSpec(50, stride, dataset)
    params = synth.make_params(50, spec.n_head_channels, spec.base_width, seed=seed, logit_gain=synth.logit_gain_for(50, stride, spec.base_width))
    return spec, Engine(spec, params, 'f16', max_batch=n, device=cuda)


def _forward_noted(lib, eng, x):
    """_forward_with_moments under metro_kernel_notes(1) -> its outputs and the ids of every launch it made."""
    check(lib.metro_kernel_notes(1), 'notes')
    try:
        out = _forward_with_moments(eng, x)
        torch.cuda.synchronize()
        return out, lib.metro_last_kernel_id().decode().split(' & ')
    finally:
        lib.metro_kernel_notes(0)


@pytest.mark.parametrize('stride,dataset,n,head', FORWARD_CASES)
def test_engine_forward_moments_on_the_wide_tile_heads(lib, cuda, stride, dataset, n, head):
    """test_engine_forward_moments at call sizes where the plan runs the 256- and 128-pixel-tile heads (max_batch = 4 there never
    reaches them): full-width synthetic nets in f16, four base crops laid out as twins.  Poses, coords01 and status words are
    the plain forward's bits; Cov01 and peak match the restatement of the forward_upto logits of the base crops; every position
    carries its twin's bits.  The launches the moments call notes are the plan's, with the MOMENTS head and finalize at the end."""
    from metro_pose3d_amd import synth
    spec, eng = _full_width_engine(cuda, stride, dataset, n)
    sk = spec.skeleton
    p = BASE_IMAGES
    assign = H.crop_assignment(n, p, zlib.crc32(f'forward/{stride}/{dataset}/{n}'.encode()))
    base = torch.from_numpy(synth.make_images(p, spec.proc_side, seed=5)).to(cuda)
    x = H.lay_out_twins(base, assign)
    plan_ids = eng.layer_kernels(n)
    assert plan_ids[-2:] == [head, 'softargmax_finalize<acc32>'], plan_ids[-2:]
    c01_plain = torch.full((n, sk.n_head, 3), float('nan'), device=cuda)
    poses_plain = eng.forward(x, coords01=c01_plain).clone()
    status_plain = eng.status_words(n).clone()
    (poses, c01, cov, peak), noted = _forward_noted(lib, eng, x)
    assert noted[-2:] == [with_moments(head), FIN], noted[-2:]
    assert noted[:-2] == [k for layer in plan_ids[:-2] for k in layer.split(' & ')], 'the backbone in front of the head is not the plan\'s'
    assert torch.equal(_bits(poses), _bits(poses_plain)) and torch.equal(_bits(c01), _bits(c01_plain))
    assert torch.equal(eng.status_words(n), status_plain) and int(status_plain.sum()) == 0
    for t, name in ((cov, 'cov01'), (peak, 'peak'), (c01, 'coords01'), (poses, 'poses')):
        H.assert_twins(t, assign, p, f'{head} ({name})')
    logits = eng.forward_upto(x, len(eng.layer_infos()) - 2)[:p].cpu().numpy()        # at the same call size: the same head kernel
    mu, cov_ref, peak_ref = _moments_by_image(logits, sk.n_head, spec.depth)
    covn, peakn = cov[:p].cpu().numpy(), peak[:p].cpu().numpy()
    _conditions(covn, peakn, head)
    dev = _deviation(covn, cov_ref, spec.heatmap_side)
    print(f'\n[{with_moments(head)}] forward, stride {stride} {dataset}, {n} crops: Cov01 deviation {dev:.3e} (bar {_fp32_bound():.3e})')
    assert dev <= _fp32_bound()
    assert np.allclose(peakn, peak_ref, rtol=1e-5)
    assert np.abs(c01[:p].cpu().numpy() - mu).max() <= 2e-6
    eng.close()


# ---- 5. non-finite inputs through each of the five moments kernels ------------------------------------------------------------
# the smallest case of this file or of tests/test_gpu_heat_moments.py:HEAD_CASES with a second crop that launches each head kernel:
# (name, c_in, stride, n, joints, id)
NF_HEADS = [
    ('head_f16_kernel', 320, 32, 2, 17, 'head_f16<160x64,moments>'),              # HEAD_CASES plain64-one-record
    ('head_f16_kernel256', 320, 4, 16, 17, 'head_f16<160x256,moments>'),          # HEAD_CASES plain256
    ('head_f16_ring_kernel', 2048, 32, 2, 17, 'head_f16<144x64,k4,moments>'),     # rn50-s32-h36m of the closure, two crops
]
POISONED = 1                    # the crop that takes the plants


def _report_poisoned(what, cov, peak, joints=None, clean=None):
    """What the poisoned crop's own moments are, printed, and held to what include/metro_hip.h states of them: six NaN words and a
    NaN peak for every joint with a NaN or +Inf logit (`joints`; None = all), the clean call's bits for the crop's other joints."""
    c, k = cov[POISONED], peak[POISONED]
    print(f'\n[{what}] poisoned crop: {int(np.isnan(c).all(-1).sum())} of {c.shape[0]} joints with six NaN covariance words, '
          f'{int(np.isnan(k).sum())} NaN peaks, {int(np.isinf(c).sum() + np.isinf(k).sum())} infinite words, '
          f'{int((np.isnan(c).any(-1) != np.isnan(c).all(-1)).sum())} joints partly NaN')
    hit = np.ones(c.shape[0], bool) if joints is None else np.isin(np.arange(c.shape[0]), joints)
    assert np.isnan(c[hit]).all() and np.isnan(k[hit]).all(), what
    if not hit.all():
        assert np.array_equal(c[~hit].view(np.int32), clean[0][POISONED][~hit].view(np.int32)), what
        assert np.array_equal(k[~hit].view(np.int32), clean[1][POISONED][~hit].view(np.int32)), what


@pytest.mark.parametrize('case', NF_HEADS, ids=[c[0] for c in NF_HEADS])
def test_nonfinite_input_through_a_moments_head(lib, cuda, case):
    """One NaN and one +Inf in one crop's input.  The crop's poses are the plain head's bits on the same input (the plain entry
    has no coords01 output); every other crop's cov01, peak and coords01 are the clean call's bits."""
    name, c_in, stride, n, nj, kid = case
    spec = ModelSpec(50, stride, {17: 'h36m', 19: 'many19', 53: 'merged'}[nj])
    side = spec.heatmap_side
    assign, p, x, params = _head_operands(spec, n, c_in, 1.0, f'nonfinite/{name}', cuda)
    x = x.clone()
    x[POISONED] = torch.randn(x[POISONED].shape, device=cuda, generator=torch.Generator(device=cuda).manual_seed(5)).half()    # a crop of its own
    clean = launch_head(lib, cuda, spec, n, c_in, x, params, logits=False)
    assert clean['ids'] == [kid, FIN], clean['ids']
    _conditions(clean['cov'].cpu().numpy(), clean['peak'].cpu().numpy(), name)
    x[POISONED, 0, 1, c_in // 2] = float('nan')
    x[POISONED, side - 1, side - 2, 3] = float('inf')
    got = launch_head(lib, cuda, spec, n, c_in, x, params, logits=False)
    plain = launch_head(lib, cuda, spec, n, c_in, x, params, moments=False, logits=False)
    assert torch.equal(_bits(got['poses']), _bits(plain['poses'])), 'poses differ from the plain head on the same input'
    assert torch.isnan(got['poses'][POISONED]).all() and torch.isnan(got['c01'][POISONED]).all()
    others = [i for i in range(n) if i != POISONED]
    for k in ('cov', 'peak', 'c01', 'poses'):
        assert torch.equal(_bits(got[k][others]), _bits(clean[k][others])), f'{kid}: {k} of a crop without a plant differs from the clean call'
    _report_poisoned(kid, got['cov'].cpu().numpy(), got['peak'].cpu().numpy())


@pytest.mark.parametrize('precise', [0, 1, 2])
def test_nonfinite_logits_through_the_two_launch_moments(lib, cuda, precise):
    """softargmax_partial / softargmax_finalize with moments at the smallest case of SA_CLOSURE_CASES (side 2, 17 joints): a NaN
    logit of joint 3 and a +Inf logit of joint 5 in one crop.  coords01 are metro_softargmax01's bits on the same logits; every
    other crop keeps the clean call's bits."""
    spec, n = SA_CLOSURE_CASES[0].values
    nj = spec.skeleton.n_head
    lg = random_logits(spec, n, 1.0, 2)
    clean = run_softargmax(lib, cuda, spec, lg, precise)
    lg[POISONED, 0, 1, 2 * nj + 3] = np.nan
    lg[POISONED, 1, 0, 7 * nj + 5] = np.inf
    c01, cov, peak, c01_plain = run_softargmax(lib, cuda, spec, lg, precise)
    assert torch.equal(_bits(c01), _bits(c01_plain)), 'coords01 differ from metro_softargmax01 on the same logits'
    bad = np.isnan(c01.cpu().numpy()).all(-1)
    assert bad.sum() == 2 and bad[POISONED, 3] and bad[POISONED, 5], np.argwhere(bad)
    others = [i for i in range(n) if i != POISONED]
    assert torch.equal(_bits(c01[others]), _bits(clean[0][others]))
    assert np.array_equal(cov[others].view(np.int32), clean[1][others].view(np.int32)) and np.array_equal(peak[others].view(np.int32), clean[2][others].view(np.int32))
    _report_poisoned(f'softargmax_partial<precise {precise},moments>', cov, peak, joints=[3, 5], clean=clean[1:3])


def test_nonfinite_crop_through_forward_moments(lib, cuda):
    """The same through metro_forward_moments (the full-width stride-32 net of test_engine_forward_moments, three crops): the
    poisoned crop's poses, coords01 and status word are the plain forward's bits on the same input, the other crops' cov01, peak
    and coords01 those of the clean call."""
    from metro_pose3d_amd import synth
    n = 3
    spec, eng = _full_width_engine(cuda, 32, 'h36m', 4)
    sk = spec.skeleton
    x = torch.from_numpy(synth.make_images(n, spec.proc_side, seed=5)).to(cuda)
    _, c01_clean, cov_clean, peak_clean = [t.clone() for t in _forward_with_moments(eng, x)]
    assert int(eng.status_words(n).sum()) == 0
    x[POISONED, 100, 37, 1] = float('nan')
    x[POISONED, 200, 150, 0] = float('inf')
    c01_plain = torch.full((n, sk.n_head, 3), float('nan'), device=cuda)
    poses_plain = eng.forward(x, coords01=c01_plain).clone()
    status_plain = eng.status_words(n).clone()
    poses, c01, cov, peak = _forward_with_moments(eng, x)
    assert torch.equal(_bits(poses), _bits(poses_plain)) and torch.equal(_bits(c01), _bits(c01_plain))
    assert torch.equal(eng.status_words(n), status_plain) and status_plain.tolist() == [0, 1, 0], status_plain.tolist()
    others = [i for i in range(n) if i != POISONED]
    for got, want, name in ((cov, cov_clean, 'cov01'), (peak, peak_clean, 'peak'), (c01, c01_clean, 'coords01')):
        assert torch.equal(_bits(got[others]), _bits(want[others])), f'{name} of a crop without a plant differs from the clean call'
    _report_poisoned('metro_forward_moments', cov.cpu().numpy(), peak.cpu().numpy())
    eng.close()
