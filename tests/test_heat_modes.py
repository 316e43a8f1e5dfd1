"""Per-joint heat-map modes without a GPU: the fp64 restatement (tests/heat_modes_ref.py) on known answers, heat_modes.hip's
kernel body compiled for the host and walked by a team of one thread (every slab, flag, round and window of modes_walk; the
workgroup's ladders are the one part only the GPU tests run), the new C symbols and their refusals, and the argument checks of
the Python surface that run before any launch.

Tolerances: profiles/heat_modes_parity.json records the worst deviation of every comparison per accumulator type (mass and
peak in probability, coords01 in grid units, cov01 relative to one voxel's variance; tools/heat_modes_parity.py); the tests
assert four times those figures (heat_modes_ref.gate).  `voxel` is always compared exactly."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

from metro_pose3d_amd import ModelSpec, _lib
from tests import heat_modes_ref as MR
from tests.helpers import compile_for_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('metro_plan_modes_scratch_bytes', 'metro_plan_bind_modes')


# ---- the restatement on known answers ------------------------------------------------------------------------------------------

def blob(s, d, centre, sigma, amp=1.0):
    """amp * N(centre, sigma^2 I) on the voxel grid [s, s, d], (y, x, d) order, normalised over the unbounded lattice."""
    y, x, z = np.meshgrid(np.arange(s), np.arange(s), np.arange(d), indexing='ij')
    r2 = (y - centre[0]) ** 2 + (x - centre[1]) ** 2 + (z - centre[2]) ** 2
    return amp * np.exp(-r2 / (2.0 * sigma ** 2)) / (2 * np.pi * sigma ** 2) ** 1.5


def one_joint(vol, k, radius):
    s, _, d = vol.shape
    voxel, stats = MR.modes(vol.reshape(1, s, s, d), 1, d, [0], k, radius)
    return voxel[0, 0], stats[0, 0]


def lin(v, s, d):
    return v // (s * d), v // d % s, v % d


def test_one_concave_blob_gives_one_mode_at_its_centre():
    s, d, k = 9, 8, 3
    y, x, z = np.meshgrid(np.arange(s), np.arange(s), np.arange(d), indexing='ij')
    vol = -0.5 * ((y - 4) ** 2 + (x - 6) ** 2 + (z - 2) ** 2.0)
    voxel, stats = one_joint(vol, k, 1)
    assert voxel.tolist() == [(4 * s + 6) * d + 2, -1, -1]
    assert np.array_equal(stats[1:, 0], [0, 0]) and np.isnan(stats[1:, 1:]).all()
    assert np.allclose(stats[0, 2:5], [MR.lin01(s)[6], MR.lin01(s)[4], MR.lin01(d)[2]], atol=1e-12)     # symmetric window
    assert 0 < stats[0, 1] < stats[0, 0] < 1 and np.allclose(stats[0, 8:], 0, atol=1e-15)


def test_two_separated_blobs_give_two_modes_and_the_mean_lies_between():
    """The case the feature exists for: log(a N1 + b N2), a > b."""
    s, d, a, b = 16, 8, 0.7, 0.3
    c1, c2 = (3, 4, 2), (12, 13, 6)
    vol = np.log(blob(s, d, c1, 0.6, a) + blob(s, d, c2, 0.6, b))
    voxel, stats = one_joint(vol, 2, 2)
    assert [lin(v, s, d) for v in voxel] == [c1, c2]
    assert abs(stats[0, 0] - a) < 2e-3 and abs(stats[1, 0] - b) < 2e-3 and stats[:, 0].sum() <= 1
    p = np.exp(vol - np.log(np.exp(vol).sum()))
    gs, gd = MR.lin01(s), MR.lin01(d)
    mean = np.array([(p.sum((0, 2)) * gs).sum(), (p.sum((1, 2)) * gs).sum(), (p.sum((0, 1)) * gd).sum()])      # the call's coords01
    assert (stats[0, 2:5] + 0.1 < mean).all() and (mean < stats[1, 2:5] - 0.1).all()                          # between the two, at neither
    assert np.abs(mean - (a * stats[0, 2:5] + b * stats[1, 2:5])).max() < 1e-3                                # their mass-weighted blend
    at = p[abs(gs - mean[1]).argmin(), abs(gs - mean[0]).argmin(), abs(gd - mean[2]).argmin()]
    assert at < 1e-9                                                                                          # nothing AT the mean


def test_a_lower_peak_within_2r_is_suppressed():
    s, d = 12, 8
    vol = np.zeros((s, s, d))
    vol[3, 3, 3], vol[3, 6, 3], vol[9, 9, 3] = 9.0, 8.0, 7.0
    assert [lin(v, s, d) for v in one_joint(vol, 3, 1)[0][:3]] == [(3, 3, 3), (3, 6, 3), (9, 9, 3)]        # 3 apart > 2R = 2
    voxel, _ = one_joint(vol, 3, 2)                                                                        # 3 apart <= 2R = 4
    assert [lin(v, s, d) for v in voxel[:2]] == [(3, 3, 3), (9, 9, 3)]
    assert (3, 6, 3) not in [lin(v, s, d) for v in voxel if v >= 0]


def test_plateaus_and_a_constant_volume_give_one_mode_at_the_lowest_index():
    s, d = 6, 4
    voxel, stats = one_joint(np.full((s, s, d), 2.5), 4, 0)
    assert voxel.tolist() == [0, -1, -1, -1] and abs(stats[0, 0] - 1.0 / (s * s * d)) < 1e-15
    vol = np.zeros((s, s, d))
    vol[2:4, 1:4, 1:3] = 5.0                                                     # a box-shaped plateau
    voxel, _ = one_joint(vol, 2, 0)
    assert lin(voxel[0], s, d) == (2, 1, 1)
    # the rest of the volume is one more plateau, but it touches the higher one: only voxels away from it can lead it
    assert voxel[1] == 0 or voxel[1] == -1


def test_a_peak_in_a_corner_has_a_clipped_window():
    s, d = 5, 4
    vol = np.zeros((s, s, d))
    vol[s - 1, s - 1, d - 1] = 3.0
    voxel, stats = one_joint(vol, 1, 1)
    assert lin(voxel[0], s, d) == (s - 1, s - 1, d - 1)
    z = np.exp(3.0) + s * s * d - 1
    assert abs(stats[0, 0] - (np.exp(3.0) + 7) / z) < 1e-14 and abs(stats[0, 1] - np.exp(3.0) / z) < 1e-14       # 2 x 2 x 2 voxels
    assert stats[0, 2] < 1 and stats[0, 3] < 1 and stats[0, 4] < 1


def test_masses_of_a_joint_sum_to_at_most_one():
    rng = np.random.default_rng(5)
    lg = rng.standard_normal((2, 8, 8, 4 * 3)) * 3
    for radius in (0, 1, 3):
        voxel, stats = MR.modes(lg, 3, 4, [0, 1, 2], 8, radius)
        assert (np.nansum(stats[..., 0], -1) <= 1 + 1e-12).all()
        assert ((voxel >= 0) == (stats[..., 0] > 0)).all()


@pytest.mark.parametrize('s,d', ((2, 4), (4, 4), (3, 2), (4, 3)))
def test_a_window_of_the_whole_volume_gives_the_forwards_moments(s, d):
    from tests import heat_moments_ref as HM
    rng = np.random.default_rng([s, d])
    lg = rng.standard_normal((2, s, s, d * 3)) * 2
    voxel, stats = MR.modes(lg, 3, d, [0, 1, 2], 2, 3)
    mu, cov, peak, _ = HM.moments(lg, 3, d)
    assert (voxel[..., 0] >= 0).all() and (voxel[..., 1] == -1).all()            # everything is within 2R of the first mode
    assert np.allclose(stats[..., 0, 0], 1, atol=1e-13) and np.allclose(stats[..., 0, 1], peak, rtol=1e-12)
    assert np.allclose(stats[..., 0, 2:5], mu, atol=1e-12) and np.allclose(stats[..., 0, 5:], HM.cov6(cov), atol=1e-12)


def test_minus_inf_voxels_are_never_modes_and_nonfinite_logits_poison_their_joint_only():
    rng = np.random.default_rng(6)
    s, d, j = 6, 4, 3
    lg = rng.standard_normal((2, s, s, d * j))
    clean = MR.modes(lg, j, d, [0, 1, 2], 3, 1)
    holes = lg.copy()
    holes[0, :, :3, 0::j] = -np.inf                                               # joint 0: the left half of every depth
    voxel, stats = MR.modes(holes, j, d, [0, 1, 2], 3, 1)
    assert all(lin(v, s, d)[1] >= 3 for v in voxel[0, 0] if v >= 0) and (voxel[0, 0] >= 0).any()
    assert np.array_equal(voxel[:, 1:], clean[0][:, 1:]) and np.array_equal(stats[:, 1:], clean[1][:, 1:])
    allinf = lg.copy()
    allinf[1, :, :, 1::j] = -np.inf
    voxel, stats = MR.modes(allinf, j, d, [0, 1, 2], 3, 1)
    assert (voxel[1, 1] == -1).all() and (stats[1, 1, :, 0] == 0).all() and np.isnan(stats[1, 1, :, 1:]).all()
    for bad in (np.nan, np.inf):
        poisoned = lg.copy()
        poisoned[1, 2, 3, 1 * j + 2] = bad
        voxel, stats = MR.modes(poisoned, j, d, [0, 1, 2], 3, 1)
        assert (voxel[1, 2] == -1).all() and np.isnan(stats[1, 2]).all()
        keep = np.ones((2, j), bool)
        keep[1, 2] = False
        assert np.array_equal(voxel[keep], clean[0][keep]) and np.array_equal(stats[keep], clean[1][keep])


# ---- heat_modes.hip compiled for the host --------------------------------------------------------------------------------------

HOST_BODY = '''
#include <vector>
struct ModesHostTeam {
    static constexpr int tid = 0, nt = 1, group = 0, n_groups = 1, lane = 0, lanes = 1;
    void sync() const {}
    template <typename T> T max(T x) const { return x; }
    template <typename T> T sum(T x) const { return x; }
    template <typename T> T group_sum(T x) const { return x; }
    template <typename L> metro::ModeCand<L> best(metro::ModeCand<L> c) const { return c; }
};
template <typename AccT, typename LogitT>
static int walk(const void* logits, int n, int side, int J, int D, const int* perm, int n_out, int K, int R, int slab_rows,
                int32_t* voxel, float* stats) {
    using namespace metro;
    ModesArgs a;
    a.logits = logits; a.voxel = voxel; a.stats = stats;
    a.side = side; a.J = J; a.D = D; a.n_out = n_out; a.K = K; a.radius = R;
    a.slab_rows = slab_rows > 0 ? slab_rows : md_slab_rows(side, D, (int)sizeof(LogitT));
    if (a.slab_rows == 0) return 0;
    for (int r = 0; r < n_out; ++r) a.perm[r] = perm[r];
    const size_t bytes = md_lds_bytes(side, D, (int)sizeof(LogitT), a.slab_rows);
    if (bytes > (size_t)MD_LDS_MAX) return -1;
    std::vector<double> lds(bytes / 8 + 1);                      // exactly the kernel's LDS image: an overrun is a host fault
    ModesHostTeam team;
    for (int img = 0; img < n; ++img)
        for (int r = 0; r < n_out; ++r) modes_walk<AccT, LogitT>(a, img, r, reinterpret_cast<char*>(lds.data()), team);
    return a.slab_rows;
}
extern "C" int host_heat_modes(const void* logits, int precise, int n, int side, int J, int D, const int* perm, int n_out, int K,
                               int R, int slab_rows, int32_t* voxel, float* stats) {
    if (precise == 0) return walk<float, float>(logits, n, side, J, D, perm, n_out, K, R, slab_rows, voxel, stats);
    if (precise == 1) return walk<double, float>(logits, n, side, J, D, perm, n_out, K, R, slab_rows, voxel, stats);
    return walk<double, double>(logits, n, side, J, D, perm, n_out, K, R, slab_rows, voxel, stats);
}
extern "C" int host_slab_rows(int side, int D, int logit_bytes) { return metro::md_slab_rows(side, D, logit_bytes); }
'''
# (side, joints, depth, crops, k, radius, slab rows: 0 = the launcher's own choice): every S, D, J, K, R and n of the issue; the maps
# that fit in LDS whole also in slabs of 1, 3 and 5 rows, which walk the halo code of the S = 64 volumes at sizes a test can afford
HOST_CASES = [(2, 1, 1, 1, 1, 0, 0), (2, 17, 4, 2, 2, 1, 0), (2, 53, 8, 1, 8, 3, 0), (3, 19, 8, 2, 2, 1, 0), (3, 53, 1, 1, 8, 0, 0),
              (3, 17, 4, 2, 1, 3, 1), (8, 17, 8, 2, 2, 1, 0), (8, 53, 4, 1, 8, 1, 3), (8, 19, 1, 2, 2, 3, 1), (8, 1, 8, 1, 8, 0, 5),
              (16, 17, 8, 2, 2, 1, 0), (16, 19, 8, 1, 8, 0, 5), (16, 1, 4, 2, 1, 3, 3), (16, 53, 8, 1, 2, 1, 1), (20, 17, 8, 1, 2, 1, 0),
              (20, 19, 4, 2, 8, 3, 3), (20, 1, 1, 1, 2, 0, 1), (64, 17, 8, 1, 2, 1, 0), (64, 1, 8, 2, 8, 3, 0), (64, 19, 4, 1, 8, 0, 0)]
ACC_KEYS = {0: 'host/acc32-logits32', 1: 'host/acc64-logits32', 2: 'host/acc64-logits64'}


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    return load_host(tmp_path_factory.mktemp('host_heat_modes'))


def load_host(tmp):
    dll = compile_for_host(tmp, 'host_heat_modes', ['heat_modes.hip'], HOST_BODY)
    dll.host_heat_modes.restype = C.c_int
    dll.host_heat_modes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_void_p, C.c_void_p]
    dll.host_slab_rows.restype = C.c_int
    dll.host_slab_rows.argtypes = [C.c_int, C.c_int, C.c_int]
    return dll


def case_permutation(j):
    """Non-identity, with a head joint left out and one repeated where there are several."""
    return [0] if j == 1 else list(range(j - 1, 0, -1)) + [j - 1]


@functools.lru_cache(maxsize=None)
def case_logits(side, j, d, n, wide):
    """Gaussian logits at gain 1 or 6 about a random level; every third case quantised to halves (exact ties and plateaus: the
    order by index decides), every fourth with a block of -Inf voxels.  fp32 values (`wide`: fp64 values that are not fp32)."""
    rng = np.random.default_rng([side, j, d, n])
    gain = (1.0, 6.0)[(side + j + n) % 2]
    lg = rng.standard_normal((n, side, side, d * j)) * gain + rng.uniform(-30, 30)
    if (side + j + d) % 3 == 0:
        lg = np.round(lg * 2) / 2
    if (side + j + d) % 4 == 0:
        lg[:, : side // 2, : side // 2, ::3] = -np.inf
    lg = np.ascontiguousarray(lg if wide else lg.astype(np.float32))
    lg.setflags(write=False)
    return lg


@functools.lru_cache(maxsize=None)
def case_reference(side, j, d, n, k, radius, wide):
    """The restatement of one case, computed once for all the tests (and precisions) that share its logits."""
    voxel, stats = MR.modes(case_logits(side, j, d, n, wide), j, d, case_permutation(j), k, radius)
    voxel.setflags(write=False)
    stats.setflags(write=False)
    return voxel, stats


def run_host(dll, lg, j, d, perm, k, radius, precise, slab_rows=0):
    n, side = lg.shape[:2]
    voxel = np.full((n, len(perm), k), -7, np.int32)
    stats = np.full((n, len(perm), k, MR.STATS), -7.0, np.float32)
    pa = np.asarray(perm, np.int32)
    used = dll.host_heat_modes(lg.ctypes.data, precise, n, side, j, d, pa.ctypes.data, len(perm), k, radius, slab_rows,
                               voxel.ctypes.data, stats.ctypes.data)
    assert used > 0, used
    return voxel, stats, used


def host_deviations(dll):
    """{key: {'prob', 'grid', 'cov'}}: the worst figures of every host comparison of this file (tools/heat_modes_parity.py)."""
    out = {}
    for precise, key in ACC_KEYS.items():
        worst = {'prob': 0.0, 'grid': 0.0, 'cov': 0.0}
        for side, j, d, n, k, radius, slab in HOST_CASES:
            lg = case_logits(side, j, d, n, precise == 2)
            _, stats, _ = run_host(dll, lg, j, d, case_permutation(j), k, radius, precise, slab)
            rv, rs = case_reference(side, j, d, n, k, radius, precise == 2)
            dev = MR.deviation(stats, rv, rs, side, d)
            worst = {m: max(worst[m], dev[m]) for m in worst}
        out[key] = worst
    return out


def test_the_cases_emit_few_modes_of_negligible_mass():
    emitted = small = 0
    for side, j, d, n, k, radius, _ in HOST_CASES:
        rv, rs = case_reference(side, j, d, n, k, radius, False)
        emitted += int((rv >= 0).sum())
        small += int(((rv >= 0) & (rs[..., 0] < MR.SMALL_MASS)).sum())
    print(f'heat_modes host cases: {small} of {emitted} emitted modes below {MR.SMALL_MASS:g}')
    assert emitted > 1000 and small < 0.05 * emitted


@pytest.mark.parametrize('precise', (0, 1, 2))
@pytest.mark.parametrize('side,j,d,n,k,radius,slab', HOST_CASES, ids=lambda v: str(v))
def test_host_compiled_kernel_code_against_the_restatement(host, side, j, d, n, k, radius, slab, precise):
    lg = case_logits(side, j, d, n, precise == 2)
    voxel, stats, used = run_host(host, lg, j, d, case_permutation(j), k, radius, precise, slab)
    assert used == (slab or host.host_slab_rows(side, d, lg.itemsize))
    rv, rs = case_reference(side, j, d, n, k, radius, precise == 2)
    MR.check(voxel, stats, rv, rs, side, d, ACC_KEYS[precise], f'S{side} J{j} D{d} n{n} K{k} R{radius} slab {used}')
    assert (np.nansum(stats[..., 0].astype(np.float64), -1) <= 1 + 1e-5).all()


def test_slab_rows_keep_every_shape_within_64_kb(host):
    """S = 64, D = 8: 32 KB of flags, and slabs of 13 (fp32) or 5 (fp64) rows plus two halo rows; a volume whose flags alone fill
    the LDS is refused (0), which the launcher turns into METRO_ERR_UNSUPPORTED."""
    assert host.host_slab_rows(64, 8, 4) == 13 and host.host_slab_rows(64, 8, 8) == 5
    assert host.host_slab_rows(16, 8, 4) == 16 and host.host_slab_rows(8, 8, 8) == 8 and host.host_slab_rows(2, 1, 4) == 2
    assert host.host_slab_rows(64, 16, 4) == 0 and host.host_slab_rows(96, 8, 8) == 0
    for s, d, b in ((64, 8, 4), (64, 8, 8), (64, 4, 8), (48, 8, 8), (32, 8, 4)):
        rows = host.host_slab_rows(s, d, b)
        assert rows > 0 and 128 + (s * s * d + 15) // 16 * 16 + min(s, rows + 2) * s * d * b <= 64 * 1024, (s, d, b, rows)


@pytest.mark.parametrize('precise', (0, 1, 2))
def test_host_compiled_code_on_the_known_answers(host, precise):
    """Every slab height gives the same bits; -Inf voxels, an all -Inf joint, and NaN / +Inf confined to their joint."""
    dt = np.float64 if precise == 2 else np.float32
    side, j, d, k, radius = 7, 3, 4, 3, 1
    rng = np.random.default_rng(11)
    lg = (rng.standard_normal((2, side, side, d * j)) * 2).astype(dt)
    lg[0, :, :3, 0::j] = -np.inf
    lg[1, :, :, 1::j] = -np.inf
    perm = [2, 0, 1]
    voxel, stats, used = run_host(host, lg, j, d, perm, k, radius, precise)
    assert used == side
    rv, rs = MR.modes(lg, j, d, perm, k, radius)
    MR.check(voxel, stats, rv, rs, side, d, ACC_KEYS[precise], 'holes')
    assert (voxel[1, 2] == -1).all() and (stats[1, 2, :, 0] == 0).all()
    for slab in (1, 2, 3, 4, 5):
        v2, s2, _ = run_host(host, lg, j, d, perm, k, radius, precise, slab)
        assert np.array_equal(v2, voxel) and np.array_equal(s2, stats, equal_nan=True), slab
    for bad in (np.nan, np.inf):
        poisoned = lg.copy()
        poisoned[1, 3, 3, 2 * j + 0] = bad
        pv, ps, _ = run_host(host, poisoned, j, d, perm, k, radius, precise, 2)
        assert (pv[1, 1] == -1).all() and np.isnan(ps[1, 1]).all(), bad
        keep = np.ones((2, 3), bool)
        keep[1, 1] = False
        assert np.array_equal(pv[keep], voxel[keep]) and np.array_equal(ps[keep], stats[keep], equal_nan=True), bad


def test_recorded_tolerances_are_the_figures_of_this_code(host):
    """The file the gates come from holds what the host comparisons give (same compiler, same libm: to 1 %), so a gate can
    only have come from a measurement."""
    rec = MR.recorded()
    for key, dev in host_deviations(host).items():
        w = rec['worst'][key]
        print(f'heat_modes {key}: ' + ' '.join(f'{m} {dev[m]:.3e} (recorded {w[m]:.3e})' for m in dev))
        assert all(dev[m] <= w[m] * 1.01 for m in dev), (key, dev, w)
    for key in rec['worst']:
        MR.gate(key)


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
    assert re.search(r'#define\s+METRO_MAX_MODES\s+8\b', raw) and re.search(r'#define\s+METRO_MAX_MODE_RADIUS\s+3\b', raw)
    assert (_lib.METRO_MAX_MODES, _lib.METRO_MAX_MODE_RADIUS) == (8, 3)
    from metro_pose3d_amd import build
    assert 'heat_modes.hip' in build.SOURCES


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
        assert lib.metro_plan_modes_scratch_bytes(plan, 3) == up(3 * side * side * c * 4)
        assert lib.metro_plan_modes_scratch_bytes(plans[_lib.METRO_PREC_F64], 3) == 256
        for bad in (0, -1, 5):
            assert lib.metro_plan_modes_scratch_bytes(plan, bad) == -1
        assert lib.metro_plan_modes_scratch_bytes(None, 1) == -1
        p = C.c_void_p(4096)
        assert lib.metro_plan_bind_modes(None, p, p, p, 1, 2, 1) == -1
        for vx, st, scr in ((None, p, p), (p, None, p), (p, p, None), (None, None, p), (None, None, None)):
            assert lib.metro_plan_bind_modes(plan, vx, st, scr, 2, 2, 1) == -1, (vx, st, scr)
            assert b'go together' in lib.metro_last_error()
        assert lib.metro_plan_bind_modes(plan, None, None, None, 0, 2, 0) == -1 and b'go together' in lib.metro_last_error()
        for bad in (0, -1, 5):
            assert lib.metro_plan_bind_modes(plan, p, p, p, bad, 2, 1) == -1 and b'max_n' in lib.metro_last_error()
        for bad in (0, -1, 9):
            assert lib.metro_plan_bind_modes(plan, p, p, p, 2, bad, 1) == -1 and b'k %d outside' % bad in lib.metro_last_error()
        for bad in (-1, 4):
            assert lib.metro_plan_bind_modes(plan, p, p, p, 2, 2, bad) == -1 and b'radius %d outside' % bad in lib.metro_last_error()
        assert lib.metro_plan_bind_modes(plan, p, p, C.c_void_p(4100), 2, 2, 1) == -1 and b'aligned' in lib.metro_last_error()
        assert lib.metro_plan_bind_modes(plan, C.c_void_p(4098), p, p, 2, 2, 1) == -1 and b'aligned' in lib.metro_last_error()
        assert lib.metro_plan_bind_modes(plan, None, None, None, 0, 0, 0) == 0            # unbinding what is not bound
        # a bound forward with n > max_n is refused before any launch (and before any pointer is read: these are not memory)
        assert lib.metro_plan_bind_params(plan, C.c_void_p(4096)) == 0
        assert lib.metro_plan_bind_modes(plan, p, p, p, 2, 8, 3) == 0
        assert lib.metro_kernel_notes(1) == 0
        assert lib.metro_forward(plan, p, 3, p, p, None) == -1 and b'bound mode buffers' in lib.metro_last_error()
        assert lib.metro_forward_coords01(plan, p, 3, p, p, p, None) == -1
        assert lib.metro_forward_u8(plan, p, 3, p, None, p, None) == -1
        assert lib.metro_forward_moments(plan, p, 0, 4, p, None, None, None, None, p, None) == -1
        assert lib.metro_forward_timed(plan, p, 3, p, p, None, (C.c_float * 64)()) == -1
        # heat-maps for enough crops bound as well: the modes' own limit still refuses
        assert lib.metro_plan_bind_heatmaps(plan, p, p, p, 4) == 0
        assert lib.metro_forward(plan, p, 3, p, p, None) == -1 and b'bound mode buffers' in lib.metro_last_error()
        assert lib.metro_last_kernel_id() == b''
        assert lib.metro_kernel_notes(0) == 0
        assert lib.metro_plan_bind_heatmaps(plan, None, None, None, 0) == 0
        assert lib.metro_plan_bind_modes(plan, None, None, None, 0, 0, 0) == 0
    finally:
        for pl in plans.values():
            lib.metro_plan_destroy(pl)


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
    names = list(inspect.signature(Engine.forward_modes).parameters)
    assert names == ['self', 'images', 'k', 'radius', 'out', 'coords01', 'cov01', 'peak', 'heat_xy', 'heat_z']
    pars = inspect.signature(Engine.forward_modes).parameters
    assert pars['k'].default == 2 and pars['radius'].default == 1 and all(pars[n].default is None for n in names[4:])
    names = list(inspect.signature(INF.estimate_pose_modes).parameters)
    assert names[:8] == ['images_tensor', 'model_path', 'k', 'radius', 'precision', 'check_finite', 'return_uncertainty',
                         'return_heatmaps']
    assert {'Modes', 'estimate_pose_modes'} <= set(M.__all__) and M.Modes is INF.Modes
    assert M.estimate_pose_modes is INF.estimate_pose_modes
    assert INF.Modes._fields == ('poses', 'covariance', 'mass', 'peak', 'voxel')
    with pytest.raises(SystemExit):
        INF.main(['--modes', '2,1'])                       # --model-path is still required: argparse exits, not "unknown flag"
    x = torch.zeros((2, 256, 256, 3))
    with pytest.raises(ValueError, match='sharded calls'):
        INF.estimate_pose_modes(x, 'nowhere.npz', shard=True)
    for kw in (dict(k=0), dict(k=9), dict(k=2.0), dict(radius=-1), dict(radius=4), dict(k=True)):
        with pytest.raises(ValueError, match='must be an int in'):
            INF.estimate_pose_modes(x, 'nowhere.npz', **kw)
    spec = ModelSpec(50, 16, 'h36m', depth=4)
    eng = Engine(spec, None, 'f16', max_batch=4)
    eng._blob, eng.device = object(), torch.device('cpu')          # past the "no parameters" check, never launched
    for kw in (dict(k=0), dict(k=9), dict(radius=-1), dict(radius=4), dict(k='2')):
        with pytest.raises(ValueError, match='must be an int in'):
            eng.forward_modes(x, **kw)
    with pytest.raises(ValueError, match='out must be'):
        eng.forward_modes(x, out=torch.zeros((2, 3, 3)))
    with pytest.raises(ValueError, match='batch 5 outside'):
        eng.forward_modes(torch.zeros((5, 256, 256, 3)))
    eng._blob = None
    eng.close()


def test_modes_to_metric_blends_to_the_plain_pose():
    """Two sharp peaks that hold all the mass: the plain pose (heatmap_to_metric of the mean, root-relative) is the mass-weighted
    blend of the two mode positions; the covariances take the scaling of the metric decode."""
    from metro_pose3d_amd import inference as INF
    from tests import heat_moments_ref as HM
    spec = ModelSpec(50, 16, 'h36m', depth=8, base_width=16)
    s, d, j = spec.heatmap_side, spec.depth, spec.skeleton.n_head
    rng = np.random.default_rng(8)
    lg = np.zeros((1, s, s, d * j))
    for jj in range(j):
        a, b = rng.integers(0, [s, s, d]), rng.integers(0, [s, s, d])
        while max(abs(a - b)) <= 2:
            b = rng.integers(0, [s, s, d])
        lg[0, a[0], a[1], a[2] * j + jj], lg[0, b[0], b[1], b[2] * j + jj] = 60.0, 59.0
    perm = list(spec.skeleton.permutation)
    voxel, stats = MR.modes(lg, j, d, perm, 2, 1)
    mu = HM.moments(lg, j, d)[0]
    m = INF.modes_to_metric(spec, torch.from_numpy(stats.astype(np.float32)), torch.from_numpy(mu.astype(np.float32)),
                            torch.from_numpy(voxel))
    assert m.poses.shape == (1, len(perm), 2, 3) and m.covariance.shape == (1, len(perm), 2, 3, 3) and m.voxel.dtype == torch.int32
    last = spec.proc_side - 1
    lrc, half = last - last % spec.stride - 1, spec.stride // 2
    mm = np.concatenate([(mu[..., :2] * lrc + half) * spec.box_size_mm / spec.proc_side, mu[..., 2:] * spec.box_size_mm], -1)
    plain = (mm - mm[:, -1:])[:, perm]
    blend = (m.mass[..., None].double() * m.poses.double()).sum(2).numpy()
    assert np.allclose(m.mass.sum(-1).numpy(), 1, atol=1e-6)
    assert np.abs(blend - plain).max() < 1e-3, np.abs(blend - plain).max()       # mm: fp32 masses and coords01, 6e-8 of 2200 mm each, a few terms
    scale = HM.metric_scale(spec)
    want = np.stack([np.stack([stats[..., 5 + HM.COV6.index((min(a, b), max(a, b)))] * scale[a] * scale[b] for b in range(3)], -1)
                     for a in range(3)], -2)
    assert np.allclose(m.covariance.numpy(), want, rtol=1e-5, atol=1e-9)
