"""Per-joint heat-map posterior under a Gaussian prior without a GPU: the fp64 restatement (tests/heat_posterior_ref.py) on
known answers (a Gaussian heat-map in closed form, two peaks, a zero precision), heat_posterior.hip's kernel body compiled for
the host and walked by a team of one thread (every pass of posterior_walk, staged and streamed; the workgroup's ladders are the
one part only the GPU tests run), the new C symbols and their refusals, the dispatch of bound forwards by dry run, and the
argument checks of the Python surface that run before any launch.

Tolerances: the fp64 instantiations are held to 1e-12 in every measure (log_evidence absolute, peak' in probability, coords01' in
grid steps, cov01' in units of one voxel's variance); the fp32 instantiation to four times the figures recorded in
profiles/heat_posterior_parity.json (tools/heat_posterior_parity.py; heat_posterior_ref.gate)."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

from metro_pose3d_amd import ModelSpec, _lib
from metro_pose3d_amd._lib import check
from tests import heat_posterior_ref as PR
from tests.helpers import compile_for_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('metro_plan_prior_scratch_bytes', 'metro_plan_bind_prior')
POST_IDS = {'f16': 'heat_posterior<acc32,logits32>', 'f32': 'heat_posterior<acc64,logits32>', 'f32m': 'heat_posterior<acc64,logits32>',
            'f64': 'heat_posterior<acc64,logits64>'}


# ---- the restatement on known answers ------------------------------------------------------------------------------------------

def one_joint(vol, mu, lam):
    """One joint's volume [S, S, D] and one prior -> its 11 posterior values."""
    s, _, d = vol.shape
    return PR.posterior(vol.reshape(1, s, s, d), 1, d, [0], PR.prior_rows(mu, lam)[None, None])[0, 0]


def gaussian_logits(s, d, centre, sigma, level=0.0):
    g = PR.grid(s, d)
    return level - 0.5 * (((g - np.asarray(centre)) / np.asarray(sigma)) ** 2).sum(-1)


def test_a_gaussian_heat_map_meets_the_closed_form():
    s, d = 64, 8
    mu_h, sig_h = np.array([0.40, 0.55, 0.5]), np.array([0.05, 0.05, 0.11])
    mu = np.array([0.46, 0.50, 0.3])
    lam = np.zeros((3, 3))
    lam[0, 0], lam[1, 1], lam[0, 1], lam[1, 0] = 1 / 0.06 ** 2, 1 / 0.08 ** 2, 80.0, 80.0
    post = one_joint(gaussian_logits(s, d, mu_h, sig_h, 3.0), mu, lam)
    lam_h = np.diag(1 / sig_h ** 2)
    cov = np.linalg.inv(lam_h + lam)
    mean = cov @ (lam_h @ mu_h + lam @ mu)
    ch, l2, m = np.diag(sig_h[:2] ** 2), lam[:2, :2], (mu_h - mu)[:2]
    a = np.eye(2) + ch @ l2
    log_ev = -0.5 * np.log(np.linalg.det(a)) - 0.5 * m @ l2 @ np.linalg.inv(a) @ m
    got_cov = PR.precision_matrix(post[5:])
    print(f'closed form: mean {np.abs(post[2:5] - mean).max():.2e}, cov {np.abs(got_cov - cov).max() / cov.max():.2e} of the largest '
          f'entry, log_evidence {post[0]:.6f} ({abs(post[0] - log_ev):.2e})')
    assert abs(log_ev + 0.738366) < 1e-6
    assert np.abs(post[2:5] - mean).max() < 1e-7
    assert np.abs(got_cov - cov).max() < 1e-3 * cov.max()
    assert abs(post[0] - log_ev) < 1e-6
    assert 0 < post[1] < 1


@pytest.mark.parametrize('s', (16, 64))
def test_two_peaks_the_prior_picks_the_one_that_agrees(s):
    d, sig = 8, np.array([0.06, 0.06, 0.11])
    vol = np.log(0.55 * np.exp(gaussian_logits(s, d, (0.30, 0.5, 0.5), sig)) + 0.45 * np.exp(gaussian_logits(s, d, (0.70, 0.5, 0.5), sig)))
    plain = one_joint(vol, (0.0, 0.0, 0.0), np.zeros((3, 3)))
    post = one_joint(vol, (0.72, 0.49, 0.0), np.diag([100.0, 100.0, 0.0]))
    print(f'S {s}: plain x {plain[2]:.4f} sd {np.sqrt(plain[5]):.4f}; posterior ({post[2]:.4f}, {post[3]:.4f}) sd_x {np.sqrt(post[5]):.4f} '
          f'evidence {np.exp(post[0]):.4f}')
    assert plain[0] == 0.0 and 0.47 <= plain[2] <= 0.49 and abs(np.sqrt(plain[5]) - 0.208) < 0.005
    assert abs(post[2] - 0.705) < 0.01 and abs(post[3] - 0.4974) < 0.01
    assert np.sqrt(post[5]) < 0.06
    assert abs(np.exp(post[0]) - 0.3255) < 1e-3
    assert post[0] <= 0


@pytest.mark.parametrize('s,d', ((2, 4), (4, 4), (3, 2), (16, 8)))
def test_a_zero_precision_gives_the_plain_moments_and_zero_evidence(s, d):
    from tests import heat_moments_ref as HM
    rng = np.random.default_rng([s, d])
    j, perm = 3, [2, 0, 1, 2]
    lg = rng.standard_normal((2, s, s, d * j)) * 2
    prior = np.zeros((2, len(perm), PR.PRIOR))
    prior[..., :3] = rng.uniform(-1, 2, (2, len(perm), 3))                  # mu is free where nothing is known
    post = PR.posterior(lg, j, d, perm, prior)
    mu, cov, peak, _ = HM.moments(lg, j, d)
    assert (post[..., 0] == 0.0).all()
    assert np.allclose(post[..., 1], peak[:, perm], rtol=1e-12) and np.allclose(post[..., 2:5], mu[:, perm], atol=1e-12)
    assert np.allclose(post[..., 5:], HM.cov6(cov)[:, perm], atol=1e-12)


def test_special_rows_of_the_restatement():
    rng = np.random.default_rng(3)
    s, d, j, perm = 5, 4, 3, [1, 2, 0]
    lg = rng.standard_normal((2, s, s, d * j))
    prior = PR.prior_rows(rng.uniform(0, 1, (2, 3, 3)), np.broadcast_to(np.diag([30.0, 20.0, 0.0]), (2, 3, 3, 3)))
    clean = PR.posterior(lg, j, d, perm, prior)
    assert np.isfinite(clean).all() and (clean[..., 0] <= 0).all()
    keep = np.ones((2, 3), bool)
    keep[1, 0] = False
    bad_prior = prior.copy()
    bad_prior[1, 0, 4] = np.nan
    got = PR.posterior(lg, j, d, perm, bad_prior)
    assert np.isnan(got[1, 0]).all() and np.array_equal(got[keep], clean[keep])
    for bad in (np.nan, np.inf):
        poisoned = lg.copy()
        poisoned[1, 2, 3, 1 * j + perm[0]] = bad
        got = PR.posterior(poisoned, j, d, perm, prior)
        assert np.isnan(got[1, 0]).all() and np.array_equal(got[keep], clean[keep]), bad
    holes = lg.copy()
    holes[0, :, :2, 0::j] = -np.inf                                           # head joint 0 = output row 2: the left columns
    got = PR.posterior(holes, j, d, perm, prior)
    assert np.isfinite(got).all() and got[0, 2, 2] > clean[0, 2, 2] and np.array_equal(got[:, :2], clean[:, :2])
    holes[0, :, :, 0::j] = -np.inf
    assert np.isnan(PR.posterior(holes, j, d, perm, prior)[0, 2]).all()


# ---- heat_posterior.hip compiled for the host ------------------------------------------------------------------------------------

HOST_BODY = '''
#include <vector>
struct PosteriorHostTeam {
    static constexpr int tid = 0, nt = 1;
    void sync() const {}
    template <int N, typename T> void maxes(T (&)[N]) const {}
    template <int N, typename T> void sums(T (&)[N]) const {}
};
template <typename AccT, typename LogitT, typename OutT>
static int walk(const void* logits, const float* prior, int n, int side, int J, int D, const int* perm, int n_out, int staged, void* post) {
    using namespace metro;
    PosteriorArgs a;
    a.logits = logits; a.prior = prior; a.post = post;
    a.side = side; a.J = J; a.D = D; a.n_out = n_out;
    const bool fits = po_fits(side, D, (int)sizeof(LogitT));
    if (staged == 1 && !fits) return -1;
    a.staged = staged < 0 ? (fits ? 1 : 0) : staged;
    for (int r = 0; r < n_out; ++r) a.perm[r] = perm[r];
    const size_t bytes = po_lds_bytes(side, D, (int)sizeof(LogitT), a.staged != 0);
    if (bytes > (size_t)PO_LDS_MAX) return -1;
    std::vector<double> lds(bytes / 8 + 1);                      // exactly the kernel's LDS image: an overrun is a host fault
    PosteriorHostTeam team;
    for (int img = 0; img < n; ++img)
        for (int r = 0; r < n_out; ++r) posterior_walk<AccT, LogitT, OutT>(a, img, r, reinterpret_cast<char*>(lds.data()), team);
    return a.staged;
}
extern "C" int host_heat_posterior(const void* logits, const float* prior, int precise, int n, int side, int J, int D, const int* perm,
                                   int n_out, int staged, int wide_out, void* post) {
    // wide_out: the accumulators' values as they are, before the one rounding to fp32 (what the 1e-12 comparisons read)
    if (precise == 0) return walk<float, float, float>(logits, prior, n, side, J, D, perm, n_out, staged, post);
    if (precise == 1 && wide_out) return walk<double, float, double>(logits, prior, n, side, J, D, perm, n_out, staged, post);
    if (precise == 1) return walk<double, float, float>(logits, prior, n, side, J, D, perm, n_out, staged, post);
    if (wide_out) return walk<double, double, double>(logits, prior, n, side, J, D, perm, n_out, staged, post);
    return walk<double, double, float>(logits, prior, n, side, J, D, perm, n_out, staged, post);
}
extern "C" int host_fits(int side, int D, int logit_bytes) { return metro::po_fits(side, D, logit_bytes) ? 1 : 0; }
'''
HOST_SIDES, HOST_DEPTHS, HOST_JOINTS = (1, 2, 3, 16, 33), (1, 8), (1, 17, 19, 53)
HOST_SHAPES = [(s, d, j) for s in HOST_SIDES for d in HOST_DEPTHS for j in HOST_JOINTS]
HOST_N = 2
SCENARIOS = ('psd', 'zero', 'singular', 'far', 'nan-mu', 'nan-logit', 'posinf-logit', 'neginf-logit')
ACC_KEYS = {0: 'host/acc32-logits32', 1: 'host/acc64-logits32', 2: 'host/acc64-logits64'}
DATASET_OF = {17: 'h36m', 19: 'many19', 53: 'merged'}


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    return load_host(tmp_path_factory.mktemp('host_heat_posterior'))


def load_host(tmp):
    dll = compile_for_host(tmp, 'host_heat_posterior', ['heat_posterior.hip'], HOST_BODY)
    dll.host_heat_posterior.restype = C.c_int
    dll.host_heat_posterior.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                        C.c_int, C.c_void_p]
    dll.host_fits.restype = C.c_int
    dll.host_fits.argtypes = [C.c_int, C.c_int, C.c_int]
    return dll


def real_permutation(j):
    """The output order of the skeleton with j head joints (17, 19 and 19 rows); one joint: itself."""
    return [0] if j == 1 else list(ModelSpec(50, 16, DATASET_OF[j]).skeleton.permutation)


def random_psd(rng, shape, scale):
    a = rng.standard_normal(shape + (3, 3))
    return np.einsum('...ab,...cb->...ac', a, a) * scale


@functools.lru_cache(maxsize=None)
def case(side, d, j, scenario, wide):
    """(logits, prior fp32 [n, Jout, 9]) of one scenario: Gaussian logits at gain 1 or 6 about a random level, fp32 values (`wide`:
    fp64 values that are not fp32); the prior rows as the device gets them."""
    rng = np.random.default_rng([side, d, j, SCENARIOS.index(scenario)])
    perm = real_permutation(j)
    n, r = HOST_N, len(perm)
    lg = rng.standard_normal((n, side, side, d * j)) * (1.0, 6.0)[(side + j) % 2] + rng.uniform(-30, 30)
    mu = rng.uniform(-0.2, 1.2, (n, r, 3))
    lam = random_psd(rng, (n, r), 40.0)
    if scenario == 'zero':
        lam = np.zeros_like(lam)
        lam[1:] = random_psd(rng, (n - 1, r), 40.0)                           # crop 0 knows nothing, crop 1 does
    elif scenario == 'singular':
        lam[..., 2, :] = lam[..., :, 2] = 0.0                                   # nothing known along z
        v = rng.standard_normal((r, 3))
        lam[1] = 60.0 * v[:, :, None] * v[:, None, :]                           # crop 1: rank one
    elif scenario == 'far':
        mu[...] = (3.0, -2.0, 0.5)
        lam[...] = np.diag([200.0, 200.0, 0.0])                                 # q between -800 and -1800 over the volume
    elif scenario == 'nan-mu':
        mu[0, 0, 1] = np.nan
        lam[1, r - 1, 0, 1] = lam[1, r - 1, 1, 0] = np.nan
    elif scenario in ('nan-logit', 'posinf-logit'):
        lg[1, side // 2, side - 1, (d - 1) * j + perm[0]] = np.nan if scenario == 'nan-logit' else np.inf
    elif scenario == 'neginf-logit':
        lg[:, : (side + 1) // 2, :, 0::j] = -np.inf                             # head joint 0: the upper rows (all of S = 1)
    lg = np.ascontiguousarray(lg if wide else lg.astype(np.float32))
    prior = PR.prior_rows(mu, lam).astype(np.float32)
    lg.setflags(write=False)
    prior.setflags(write=False)
    return lg, prior


@functools.lru_cache(maxsize=None)
def case_reference(side, d, j, scenario, wide):
    lg, prior = case(side, d, j, scenario, wide)
    ref = PR.posterior(lg, j, d, real_permutation(j), prior)
    ref.setflags(write=False)
    return ref


def run_host(dll, lg, prior, j, d, perm, precise, staged=-1, wide_out=False):
    """-> (post, 1 if the volume was staged in the LDS image else 0).  wide_out (fp64 accumulators only): the 11 values as fp64,
    before the one rounding to fp32 of the kernel's store."""
    n, side = lg.shape[:2]
    assert not (wide_out and precise == 0)
    post = np.full((n, len(perm), PR.STATS), -7.0, np.float64 if wide_out else np.float32)
    pa = np.asarray(perm, np.int32)
    prior = np.ascontiguousarray(prior, np.float32)
    used = dll.host_heat_posterior(lg.ctypes.data, prior.ctypes.data, precise, n, side, j, d, pa.ctypes.data, len(perm), staged,
                                   int(wide_out), post.ctypes.data)
    assert used >= 0, used
    return post, used


def host_deviations(dll):
    """{key: {measure: worst}} of every host comparison of this file (tools/heat_posterior_parity.py)."""
    out = {}
    for precise, key in ACC_KEYS.items():
        worst = dict.fromkeys(PR.MEASURES, 0.0)
        for side, d, j in HOST_SHAPES:
            for scenario in SCENARIOS:
                lg, prior = case(side, d, j, scenario, precise == 2)
                post, _ = run_host(dll, lg, prior, j, d, real_permutation(j), precise, wide_out=precise != 0)
                dev = PR.deviation(post, case_reference(side, d, j, scenario, precise == 2), side, d)
                worst = {m: max(worst[m], dev[m]) for m in worst}
        out[key] = worst
    return out


def host_bound(precise):
    return PR.gate(ACC_KEYS[0]) if precise == 0 else dict.fromkeys(PR.MEASURES, PR.EXACT)


@pytest.mark.parametrize('precise', (0, 1, 2))
@pytest.mark.parametrize('side,d,j', HOST_SHAPES, ids=lambda v: str(v))
def test_host_compiled_kernel_code_against_the_restatement(host, side, d, j, precise):
    perm = real_permutation(j)
    fits = bool(host.host_fits(side, d, 8 if precise == 2 else 4))
    assert fits == (side * side * d * (8 if precise == 2 else 4) + 256 <= 65536)
    for scenario in SCENARIOS:
        lg, prior = case(side, d, j, scenario, precise == 2)
        ref = case_reference(side, d, j, scenario, precise == 2)
        post, used = run_host(host, lg, prior, j, d, perm, precise)
        assert used == int(fits)
        if precise == 0:
            PR.check(post, ref, side, d, host_bound(precise), ACC_KEYS[precise], f'S{side} D{d} J{j} {scenario}')
        else:                       # the accumulators' values at 1e-12; what the kernel stores is their one rounding to fp32
            wide, _ = run_host(host, lg, prior, j, d, perm, precise, wide_out=True)
            PR.check(wide, ref, side, d, host_bound(precise), ACC_KEYS[precise], f'S{side} D{d} J{j} {scenario}')
            assert np.array_equal(post, wide.astype(np.float32), equal_nan=True), scenario
        streamed, _ = run_host(host, lg, prior, j, d, perm, precise, 0)          # the same order from memory: the same bits
        assert np.array_equal(streamed, post, equal_nan=True), scenario
        if fits:
            assert np.array_equal(run_host(host, lg, prior, j, d, perm, precise, 1)[0], post, equal_nan=True), scenario
        # the rows that must be NaN and those that must not
        nan_rows = np.isnan(post).any(-1)
        assert np.array_equal(nan_rows, np.isnan(post).all(-1)) and np.array_equal(nan_rows, np.isnan(ref).any(-1)), scenario
        if scenario == 'zero':
            assert (post[0, :, 0] == 0.0).all() and not np.signbit(post[0, :, 0]).any()
        if scenario == 'far':
            assert np.isfinite(post).all() and (post[..., 0] < -700).all() and (post[..., 0] > -2000).all()
        if scenario == 'nan-mu':
            want = np.zeros((HOST_N, len(perm)), bool)
            want[0, 0] = want[1, len(perm) - 1] = True
            assert np.array_equal(nan_rows, want)
        if scenario in ('nan-logit', 'posinf-logit'):
            want = np.zeros((HOST_N, len(perm)), bool)
            want[1] = [p == perm[0] for p in perm]
            assert np.array_equal(nan_rows, want)
        if scenario == 'neginf-logit':
            assert nan_rows.any() == (side == 1 and 0 in perm)


def test_one_shape_is_staged_whole_and_one_streams(host):
    """S <= 32 at D = 8 fits the LDS with fp32 logits; S = 64 does not, nor does S = 33 with fp64 logits."""
    assert host.host_fits(32, 8, 4) == 1 and host.host_fits(16, 8, 8) == 1 and host.host_fits(33, 8, 4) == 1
    assert host.host_fits(64, 8, 4) == 0 and host.host_fits(33, 8, 8) == 0 and host.host_fits(32, 8, 8) == 0
    lg, prior = case(33, 8, 17, 'psd', True)
    assert run_host(host, lg, prior, 17, 8, real_permutation(17), 2)[1] == 0
    lg, prior = case(33, 8, 17, 'psd', False)
    assert run_host(host, lg, prior, 17, 8, real_permutation(17), 1)[1] == 1


def test_host_compiled_code_on_the_two_peaks(host):
    """The case the feature exists for, through the code that ships (S = 64 streams, S = 16 is staged)."""
    for s in (16, 64):
        d, sig = 8, np.array([0.06, 0.06, 0.11])
        vol = np.log(0.55 * np.exp(gaussian_logits(s, d, (0.30, 0.5, 0.5), sig)) + 0.45 * np.exp(gaussian_logits(s, d, (0.70, 0.5, 0.5), sig)))
        prior = PR.prior_rows((0.72, 0.49, 0.0), np.diag([100.0, 100.0, 0.0]))[None, None]
        for precise in (0, 1, 2):
            lg = np.ascontiguousarray(vol.reshape(1, s, s, d), np.float64 if precise == 2 else np.float32)
            post, used = run_host(host, lg, prior, 1, d, [0], precise)
            assert used == int(s == 16)
            assert abs(post[0, 0, 2] - 0.705) < 0.01 and np.sqrt(post[0, 0, 5]) < 0.06 and abs(np.exp(post[0, 0, 0]) - 0.3255) < 1e-3


def test_recorded_tolerances_are_the_figures_of_this_code(host):
    """The file the gates come from holds what the fp32 host comparisons give (same compiler, same libm: to 1 %), so a gate can
    only have come from a measurement; the fp64 instantiations (recorded before their rounding to fp32) stay within 1e-12."""
    rec = PR.recorded()
    for key, dev in host_deviations(host).items():
        w = rec['worst'][key]
        print(f'heat_posterior {key}: ' + ' '.join(f'{m} {dev[m]:.3e} (recorded {w[m]:.3e})' for m in dev))
        if key == ACC_KEYS[0]:
            assert all(dev[m] <= w[m] * 1.01 for m in dev), (key, dev, w)
        else:
            assert all(dev[m] <= PR.EXACT and w[m] <= PR.EXACT for m in dev), (key, dev, w)
    for key in rec['worst']:
        PR.gate(key)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------

def test_new_symbols_in_header_bindings_and_library(lib):
    raw = open(os.path.join(ROOT, 'include', 'metro_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    declared = set(re.findall(r'\b(metro_[a-z0-9_]+)\s*\(', text))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        params = re.search(r'\b' + name + r'\s*\(([^)]*)\)', text).group(1)
        assert len(_lib.SIGNATURES[name][1]) == params.count(',') + 1, name
        assert 'stream' not in params, name                    # binding is host state: no launching entry was added
    assert lib.metro_abi_version() == 8 == _lib.ABI_VERSION
    assert re.search(r'#define\s+METRO_ABI_VERSION\s+8\b', raw)
    from metro_pose3d_amd import build
    assert 'heat_posterior.hip' in build.SOURCES


def test_c_refusals(lib):
    spec = ModelSpec(50, 16, 'h36m', base_width=16)
    plans = {}
    try:
        for prec in (_lib.METRO_PREC_F16, _lib.METRO_PREC_F64):
            plans[prec] = C.c_void_p()
            cs = spec.to_c(prec)
            assert lib.metro_plan_create(C.byref(cs), 4, C.byref(plans[prec])) == 0
        plan = plans[_lib.METRO_PREC_F16]
        side, c = spec.heatmap_side, spec.n_head_channels
        up = lambda v: (v + 255) // 256 * 256
        # the one-launch head keeps its logits on chip: the scratch holds them as fp32; the parity plans read the workspace
        assert lib.metro_plan_prior_scratch_bytes(plan, 3) == up(3 * side * side * c * 4)
        assert lib.metro_plan_prior_scratch_bytes(plans[_lib.METRO_PREC_F64], 3) == 256
        for bad in (0, -1, 5):
            assert lib.metro_plan_prior_scratch_bytes(plan, bad) == -1
        assert lib.metro_plan_prior_scratch_bytes(None, 1) == -1
        p = C.c_void_p(4096)
        assert lib.metro_plan_bind_prior(None, p, p, p, 1) == -1
        for pr, po, scr in ((None, p, p), (p, None, p), (p, p, None), (None, None, p), (None, None, None)):
            assert lib.metro_plan_bind_prior(plan, pr, po, scr, 2) == -1, (pr, po, scr)
            assert b'go together' in lib.metro_last_error()
        for bad in (0, -1, 5):
            assert lib.metro_plan_bind_prior(plan, p, p, p, bad) == -1 and b'max_n' in lib.metro_last_error()
        assert lib.metro_plan_bind_prior(plan, p, p, C.c_void_p(4100), 2) == -1 and b'aligned' in lib.metro_last_error()
        assert lib.metro_plan_bind_prior(plan, C.c_void_p(4098), p, p, 2) == -1 and b'aligned' in lib.metro_last_error()
        assert lib.metro_plan_bind_prior(plan, p, C.c_void_p(4097), p, 2) == -1 and b'aligned' in lib.metro_last_error()
        assert lib.metro_plan_bind_prior(plan, None, None, None, 0) == 0              # unbinding what is not bound
        # a bound forward with n > max_n is refused before any launch (and before any pointer is read: these are not memory)
        assert lib.metro_plan_bind_params(plan, C.c_void_p(4096)) == 0
        assert lib.metro_plan_bind_prior(plan, p, p, p, 2) == 0
        assert lib.metro_kernel_notes(1) == 0
        assert lib.metro_forward(plan, p, 3, p, p, None) == -1 and b'bound prior buffers' in lib.metro_last_error()
        assert lib.metro_forward_coords01(plan, p, 3, p, p, p, None) == -1
        assert lib.metro_forward_u8(plan, p, 3, p, None, p, None) == -1
        assert lib.metro_forward_moments(plan, p, 0, 4, p, None, None, None, None, p, None) == -1
        assert lib.metro_forward_timed(plan, p, 3, p, p, None, (C.c_float * 64)()) == -1
        # heat-maps and modes for enough crops bound as well: the prior's own limit still refuses
        assert lib.metro_plan_bind_heatmaps(plan, p, p, p, 4) == 0
        assert lib.metro_plan_bind_modes(plan, p, p, p, 4, 2, 1) == 0
        assert lib.metro_forward(plan, p, 3, p, p, None) == -1 and b'bound prior buffers' in lib.metro_last_error()
        assert lib.metro_last_kernel_id() == b''
        assert lib.metro_kernel_notes(0) == 0
        assert lib.metro_plan_bind_heatmaps(plan, None, None, None, 0) == 0
        assert lib.metro_plan_bind_modes(plan, None, None, None, 0, 0, 0) == 0
        assert lib.metro_plan_bind_prior(plan, None, None, None, 0) == 0
    finally:
        for pl in plans.values():
            lib.metro_plan_destroy(pl)


# ---- the dispatch of bound forwards, by dry run ----------------------------------------------------------------------------------

_DRY = C.c_void_p(4096)         # any non-NULL, 256-byte aligned pointer: a dry run launches nothing


def dry_forward_ids(lib, plan, n, entry='metro_forward'):
    check(lib.metro_kernel_notes(2), 'metro_kernel_notes')
    try:
        if entry == 'metro_forward':
            check(lib.metro_forward(plan, _DRY, int(n), _DRY, _DRY, None), 'metro_forward (dry run)')
        else:                       # an entry that always makes plain launches: what an unbound forward enqueues
            check(lib.metro_forward_moments(plan, _DRY, 0, int(n), _DRY, None, None, None, None, _DRY, None), 'metro_forward_moments (dry run)')
        return lib.metro_last_kernel_id().decode()
    finally:
        lib.metro_kernel_notes(0)


@pytest.mark.parametrize('precision', ('f16', 'f32', 'f32m', 'f64'))
def test_dispatch_of_bound_forwards_by_dry_run(lib, precision):
    """At every call size 1 .. 256: bound, heat_posterior<..> follows the finalize launch -- and the marginal and modes launches
    when those are bound too -- and nothing else changes; unbound, the kernel list is the plan's."""
    from metro_pose3d_amd.engine import Engine
    from tests.test_gpu_heat_marginals import HEAT_IDS
    from tests.test_gpu_heat_modes import MODES_IDS
    eng = Engine(ModelSpec(50, 16, 'h36m'), None, precision, max_batch=256)
    plan, post = eng._plan, POST_IDS[precision]
    check(lib.metro_plan_bind_params(plan, _DRY), 'metro_plan_bind_params')
    try:
        for n in range(1, 257):
            plain = ' & '.join(eng.layer_kernels(n))
            assert plain.endswith('>') and 'heat_' not in plain
            assert dry_forward_ids(lib, plan, n, 'metro_forward_moments') == plain, n
            check(lib.metro_plan_bind_prior(plan, _DRY, _DRY, _DRY, 256), 'bind')
            assert dry_forward_ids(lib, plan, n) == plain + ' & ' + post, n        # metro_forward itself: no captured forward
            assert dry_forward_ids(lib, plan, n, 'metro_forward_moments') == plain + ' & ' + post, n
            check(lib.metro_plan_bind_heatmaps(plan, _DRY, _DRY, _DRY, 256), 'bind')
            assert dry_forward_ids(lib, plan, n) == plain + ' & ' + HEAT_IDS[precision] + ' & ' + post, n
            check(lib.metro_plan_bind_modes(plan, _DRY, _DRY, _DRY, 256, 2, 1), 'bind')
            assert dry_forward_ids(lib, plan, n) == ' & '.join((plain, HEAT_IDS[precision], MODES_IDS[precision], post)), n
            check(lib.metro_plan_bind_heatmaps(plan, None, None, None, 0), 'unbind')
            assert dry_forward_ids(lib, plan, n) == ' & '.join((plain, MODES_IDS[precision], post)), n
            check(lib.metro_plan_bind_modes(plan, None, None, None, 0, 0, 0), 'unbind')
            check(lib.metro_plan_bind_prior(plan, None, None, None, 0), 'unbind')
            assert dry_forward_ids(lib, plan, n, 'metro_forward_moments') == plain, n
    finally:
        lib.metro_plan_bind_heatmaps(plan, None, None, None, 0)
        lib.metro_plan_bind_modes(plan, None, None, None, 0, 0, 0)
        lib.metro_plan_bind_prior(plan, None, None, None, 0)
        eng.close()


def test_plan_dispatch_is_unchanged():
    """A plan's layer kernels (the default forward) carry none of the new kernels."""
    from metro_pose3d_amd.engine import Engine
    eng = Engine(ModelSpec(50, 16, 'h36m'), None, 'f16', max_batch=64)
    ids = eng.layer_kernels(64)
    assert not any('heat_' in k for k in ids) and ids[-1] == 'softargmax_finalize<acc32>', ids[-2:]
    eng.close()


# ---- the Python surface ----------------------------------------------------------------------------------------------------------

def test_python_surface_checks_arguments_without_a_gpu():
    import metro_pose3d_amd as M
    from metro_pose3d_amd import inference as INF
    from metro_pose3d_amd.engine import Engine
    names = list(inspect.signature(Engine.forward_posterior).parameters)
    assert names == ['self', 'images', 'prior', 'out', 'coords01', 'cov01', 'peak', 'heat_xy', 'heat_z']
    assert all(inspect.signature(Engine.forward_posterior).parameters[n].default is None for n in names[3:])
    names = list(inspect.signature(INF.estimate_pose_posterior).parameters)
    assert names[:8] == ['images_tensor', 'model_path', 'prior_positions', 'prior_precision', 'precision', 'check_finite',
                         'return_uncertainty', 'return_heatmaps']
    new = {'Posterior', 'estimate_pose_posterior', 'pose_prior', 'posterior_to_metric'}
    assert new <= set(M.__all__) and all(getattr(M, k) is getattr(INF, k) for k in new)
    assert INF.Posterior._fields == ('poses', 'positions', 'covariance', 'log_evidence', 'peak')
    with pytest.raises(SystemExit):
        INF.main(['--prior', 'prior.npz'])                 # --model-path is still required: argparse exits, not "unknown flag"
    x = torch.zeros((2, 256, 256, 3))
    pos, lam = np.zeros((2, 17, 3)), np.broadcast_to(np.diag([1e-4, 1e-4, 0.0]), (2, 17, 3, 3)).copy()
    with pytest.raises(ValueError, match='sharded calls'):
        INF.estimate_pose_posterior(x, 'nowhere.npz', pos, lam, shard=True)
    skew, indefinite = lam.copy(), lam.copy()
    skew[1, 3, 0, 1] = 2e-5
    indefinite[0, 5] = np.diag([1e-4, -1e-6, 0.0])
    for kw, match in ((dict(prior_positions=pos[:1]), 'prior precision must be'), (dict(prior_positions=pos[..., :2]), r'must be \[n, Jout, 3\]'),
                      (dict(prior_precision=lam[..., 0]), 'prior precision must be'), (dict(prior_positions=pos.astype(np.int32)), 'float type'),
                      (dict(prior_positions='here'), 'torch.Tensor or numpy'), (dict(prior_positions=pos[:1], prior_precision=lam[:1]), 'holds 1 crops'),
                      (dict(prior_precision=skew), 'crop 1, joint 3 is not symmetric'),
                      (dict(prior_precision=indefinite), 'crop 0, joint 5 is not positive semi-definite')):
        args = dict(prior_positions=pos, prior_precision=lam)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            INF.estimate_pose_posterior(x, 'nowhere.npz', **args)
    spec = ModelSpec(50, 16, 'h36m')
    for bad in (skew, indefinite):
        with pytest.raises(ValueError, match='is not'):
            INF.pose_prior(spec, pos, bad)
    nan_row = lam.copy()
    nan_row[0, 0] = np.nan                                  # the caller's way to poison a joint: passed on to the device
    assert torch.isnan(INF.pose_prior(spec, pos, nan_row)[0, 0, 3:]).all()
    with pytest.raises(ValueError, match='post must be'):
        INF.posterior_to_metric(spec, torch.zeros((2, 17, 10)))
    with pytest.raises(ValueError, match='coords01'):
        INF.posterior_to_metric(ModelSpec(50, 16, 'merged'), torch.zeros((2, 19, 11)))
    eng = Engine(ModelSpec(50, 16, 'h36m', depth=4), None, 'f16', max_batch=4)
    eng._blob, eng.device = object(), torch.device('cpu')          # past the "no parameters" check, never launched
    good = torch.zeros((2, 17, 9))
    for bad in (good[:1], good[..., :8], good.double(), good.numpy(), None):
        with pytest.raises(ValueError, match='prior must be a float32 tensor'):
            eng.forward_posterior(x, bad)
    with pytest.raises(ValueError, match='out must be'):
        eng.forward_posterior(x, good, out=torch.zeros((2, 3, 3)))
    with pytest.raises(ValueError, match='batch 5 outside'):
        eng.forward_posterior(torch.zeros((5, 256, 256, 3)), torch.zeros((5, 17, 9)))
    eng._blob = None
    eng.close()


def test_pose_prior_and_posterior_to_metric_are_exact_inverses_on_fp32_values():
    """coords01 in sixteenths: their mm are fp32 values (239 * 2200 / 256 per unit), so mm -> prior -> mm returns every bit; the
    precision takes diag(a) L diag(a) in fp64 with one rounding, the covariance the same scaling."""
    from metro_pose3d_amd import inference as INF
    from tests import heat_moments_ref as HM
    spec = ModelSpec(50, 16, 'h36m')
    nj = spec.skeleton.n_out
    rng = np.random.default_rng(4)
    c01 = rng.integers(0, 17, (3, nj, 3)) / 16.0
    cov6 = rng.integers(1, 64, (3, nj, 6)) / 4096.0
    post = np.concatenate([-rng.integers(0, 8, (3, nj, 1)) / 4.0, rng.integers(1, 16, (3, nj, 1)) / 16.0, c01, cov6], -1).astype(np.float32)
    out = INF.posterior_to_metric(spec, torch.from_numpy(post))
    scale = HM.metric_scale(spec)
    half = spec.stride // 2 * spec.box_size_mm / spec.proc_side
    want = c01 * scale + np.array([half, half, 0.0])
    assert np.array_equal(out.positions.double().numpy(), want)                       # exactly representable
    root = list(spec.skeleton.permutation).index(spec.skeleton.n_head - 1)
    assert np.array_equal(out.poses.numpy(), (want - want[:, root:root + 1]).astype(np.float32))
    assert torch.equal(out.log_evidence, torch.from_numpy(post[..., 0])) and torch.equal(out.peak, torch.from_numpy(post[..., 1]))
    want_cov = (PR.precision_matrix(cov6) * (scale[:, None] * scale[None, :])).astype(np.float32)
    assert np.array_equal(out.covariance.numpy(), want_cov)
    lam_mm = PR.precision_matrix(rng.integers(1, 64, (3, nj, 6)) / 2.0 ** 20)
    prior = INF.pose_prior(spec, out.positions.numpy(), lam_mm + np.eye(3) * 2.0 ** -12)           # host arrays: checked, and PSD
    assert prior.dtype == torch.float32 and tuple(prior.shape) == (3, nj, 9)
    assert np.array_equal(prior[..., :3].numpy(), c01.astype(np.float32))             # the round trip, every bit
    l01 = (lam_mm + np.eye(3) * 2.0 ** -12) * (scale[:, None] * scale[None, :])
    assert np.array_equal(prior[..., 3:].numpy(), np.stack([l01[..., a, b] for a, b in PR.COV6], -1).astype(np.float32))
    same = INF.pose_prior(spec, out.positions, torch.from_numpy(lam_mm + np.eye(3) * 2.0 ** -12))
    assert torch.equal(same, prior)
    # the merged skeleton's output order does not carry the root head joint: the root's plain mean, from the call's coords01
    merged = ModelSpec(50, 16, 'merged')
    c_head = torch.from_numpy((rng.integers(0, 17, (3, merged.skeleton.n_head, 3)) / 16.0).astype(np.float32))
    post19 = torch.from_numpy(np.concatenate([post[:, :1], post[:, :1], post], 1)[:, :merged.skeleton.n_out].copy())
    m = INF.posterior_to_metric(merged, post19, c_head)
    root_mm = c_head[:, -1].double().numpy() * scale + np.array([half, half, 0.0])
    assert np.array_equal(m.poses.numpy(), (m.positions.double().numpy() - root_mm[:, None]).astype(np.float32))
