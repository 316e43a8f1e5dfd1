"""Per-joint heat-map marginals without a GPU: the fp64 restatement (tests/heat_marginals_ref.py) on known answers,
heat_marginals.hip's per-item arithmetic compiled for the host and walked tile by tile as its kernels walk it, the new C symbols
and their refusals, and the argument checks of the Python surface that run before any launch.

Tolerances: profiles/heat_marginals_parity.json records the worst deviation (absolute, in probability; and relative to the
row's largest entry) of every comparison, per accumulator type here; the tests assert four times that figure
(heat_marginals_ref.gate), which must stay below the probability of one voxel of a flat map."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from metro_pose3d_amd import ModelSpec, _lib
from tests import heat_marginals_ref as HR
from tests.helpers import compile_for_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('metro_plan_heatmaps_scratch_bytes', 'metro_plan_bind_heatmaps')
S, D, J = 5, 4, 3
IDENT = list(range(J))


def _volume(fill=0.0, n=1):
    return np.full((n, S, S, D * J), fill, np.float64)


# ---- the restatement on known answers ----------------------------------------------------------------------------------------

def test_constant_logits_give_flat_marginals():
    xy, z = HR.marginals(_volume(3.0), J, D, IDENT)
    assert np.allclose(xy, 1.0 / (S * S), rtol=1e-14) and np.allclose(z, 1.0 / D, rtol=1e-14)
    assert np.allclose(HR.expectations(xy, z), 0.5, atol=1e-7)


def test_one_large_logit_gives_a_delta_at_its_voxel():
    lg = _volume()
    voxels = [(0, 0, 0), (2, 4, 1), (S - 1, 1, D - 1)]
    for j, (y, x, d) in enumerate(voxels):
        lg[0, y, x, d * J + j] = 40.0
    xy, z = HR.marginals(lg, J, D, IDENT)
    for j, (y, x, d) in enumerate(voxels):
        assert abs(xy[0, j, y, x] - 1) < 1e-15 and abs(z[0, j, d] - 1) < 1e-15
        assert xy[0, j].sum() - xy[0, j, y, x] < 1e-15 and z[0, j].sum() - z[0, j, d] < 1e-15
        assert np.allclose(HR.expectations(xy, z)[0, j], [HR.lin01(S)[x], HR.lin01(S)[y], HR.lin01(D)[d]], atol=1e-14)


def test_two_equal_peaks_are_both_in_the_map_and_the_mean_lies_between():
    lg = _volume()
    lg[0, 1, 0, 0 * J + 1] = lg[0, 1, 4, 3 * J + 1] = 40.0
    xy, z = HR.marginals(lg, J, D, IDENT)
    assert abs(xy[0, 1, 1, 0] - 0.5) < 1e-15 and abs(xy[0, 1, 1, 4] - 0.5) < 1e-15
    assert abs(z[0, 1, 0] - 0.5) < 1e-15 and abs(z[0, 1, 3] - 0.5) < 1e-15
    mean = HR.expectations(xy, z)[0, 1]
    assert np.allclose(mean, [0.5, HR.lin01(S)[1], 0.5], atol=1e-14) and xy[0, 1, 1, 2] < 1e-15      # nothing AT the mean


def test_permutation_moves_rows_not_values():
    rng = np.random.default_rng(3)
    lg = rng.standard_normal((2, S, S, D * J)) * 2
    xy, z = HR.marginals(lg, J, D, IDENT)
    perm = [2, 0, 2, 1]
    pxy, pz = HR.marginals(lg, J, D, perm)
    assert pxy.shape == (2, 4, S, S) and pz.shape == (2, 4, D)
    assert np.array_equal(pxy, xy[:, perm]) and np.array_equal(pz, z[:, perm])
    assert np.allclose(pxy.sum((2, 3)), 1, rtol=1e-13) and np.allclose(pz.sum(2), 1, rtol=1e-13)


def test_shifted_logits_give_the_same_maps():
    rng = np.random.default_rng(4)
    lg = rng.standard_normal((1, S, S, D * J)) * 3
    xy, z = HR.marginals(lg, J, D, IDENT)
    for shift in (80.0, -80.0):
        sxy, sz = HR.marginals(lg + shift, J, D, IDENT)
        assert np.allclose(sxy, xy, rtol=1e-12, atol=0) and np.allclose(sz, z, rtol=1e-12, atol=0)


def test_nan_logit_makes_only_its_joints_rows_nan():
    rng = np.random.default_rng(5)
    lg = rng.standard_normal((2, S, S, D * J))
    clean_xy, clean_z = HR.marginals(lg, J, D, IDENT)
    lg[1, 2, 3, 1 * J + 2] = np.nan
    xy, z = HR.marginals(lg, J, D, IDENT)
    assert np.isnan(xy[1, 2]).all() and np.isnan(z[1, 2]).all()
    keep = np.ones((2, J), bool)
    keep[1, 2] = False
    assert np.array_equal(xy[keep], clean_xy[keep]) and np.array_equal(z[keep], clean_z[keep])


# ---- heat_marginals.hip compiled for the host --------------------------------------------------------------------------------

HOST_BODY = '''
#include <vector>
template <typename AccT, typename LogitT>
static void walk(const LogitT* logits, int n, int side, int J, int D, const int* perm, int n_out, float* xy, float* z) {
    using namespace metro;
    const int pixels = side * side, C = D * J, tiles = hm_tiles(pixels), tp = hm_tile_pixels(pixels);
    const int chunk = hm_chunk_pixels(pixels, C, (int)sizeof(AccT));
    std::vector<AccT> part((size_t)tiles * C * 2), chan((size_t)C * 2), jst((size_t)J * 2), prob((size_t)chunk * C);
    std::vector<float> sums((size_t)J * tp);
    for (int img = 0; img < n; ++img) {
        const LogitT* lg = logits + (size_t)img * pixels * C;
        for (int t = 0; t < tiles; ++t) {                       // heat_partial: block (t, img), thread c
            const int p0 = t * tp, npix = pixels - p0 < tp ? pixels - p0 : tp;
            for (int c = 0; c < C; ++c)
                hm_tile_channel<AccT, LogitT>(lg + (size_t)p0 * C, C, npix, c, part[((size_t)t * C + c) * 2], part[((size_t)t * C + c) * 2 + 1]);
        }
        for (int c = 0; c < C; ++c) hm_fold<AccT>(part.data() + c * 2, tiles, (size_t)C, chan[c * 2], chan[c * 2 + 1]);      // heat_fold
        for (int j = 0; j < J; ++j) {
            AccT M, S;
            hm_fold<AccT>(chan.data() + j * 2, D, (size_t)J, M, S);
            jst[j * 2] = M; jst[j * 2 + 1] = (AccT)1 / S;
        }
        for (int idx = 0; idx < n_out * D; ++idx)
            z[(size_t)img * n_out * D + idx] = hm_z<AccT>(chan.data(), jst.data(), J, perm[idx / D], idx % D);
        for (int t = 0; t < tiles; ++t) {                       // heat_xy: block (t, img)
            const int p0 = t * tp, npix = pixels - p0 < tp ? pixels - p0 : tp;
            for (int q0 = 0; q0 < npix; q0 += chunk) {
                const int nq = npix - q0 < chunk ? npix - q0 : chunk;
                for (int idx = 0; idx < nq * C; ++idx) {
                    const int j = (idx % C) % J;
                    prob[idx] = hm_prob<AccT, LogitT>(lg[(size_t)(p0 + q0) * C + idx], jst[j * 2], jst[j * 2 + 1]);
                }
                for (int idx = 0; idx < nq * J; ++idx)
                    sums[(idx % J) * tp + q0 + idx / J] = hm_depth_sum<AccT>(prob.data() + (size_t)(idx / J) * C, J, D, idx % J);
            }
            for (int idx = 0; idx < n_out * npix; ++idx)
                xy[((size_t)img * n_out + idx / npix) * pixels + p0 + idx % npix] = sums[perm[idx / npix] * tp + idx % npix];
        }
    }
}
extern "C" int host_heat_marginals(const void* logits, int precise, int n, int side, int J, int D, const int* perm, int n_out,
                                   float* xy, float* z) {
    if (precise == 0) walk<float, float>(static_cast<const float*>(logits), n, side, J, D, perm, n_out, xy, z);
    else if (precise == 1) walk<double, float>(static_cast<const float*>(logits), n, side, J, D, perm, n_out, xy, z);
    else walk<double, double>(static_cast<const double*>(logits), n, side, J, D, perm, n_out, xy, z);
    return metro::hm_tiles(side * side);
}
extern "C" int host_tile_pixels(int pixels) { return metro::hm_tile_pixels(pixels); }
extern "C" int host_chunk_pixels(int pixels, int C, int acc_bytes) { return metro::hm_chunk_pixels(pixels, C, acc_bytes); }
'''
SIDES = (2, 3, 7, 16, 24)
HEADS = ((17, 8), (19, 8), (53, 8), (17, 4), (1, 4))
# every (side, head) pair at n = 2; n = 1 and n = 65 on one head per side (n = 65 of the widest head on the small maps only)
HOST_CASES = [(s, j, d, 2) for s in SIDES for j, d in HEADS] + \
             [(s, *HEADS[k % len(HEADS)], 1) for k, s in enumerate(SIDES)] + \
             [(2, 53, 8, 65), (3, 19, 8, 65), (7, 17, 4, 65), (16, 1, 4, 65), (24, 17, 8, 65)]
ACC_KEYS = {0: 'host/acc32-logits32', 1: 'host/acc64-logits32', 2: 'host/acc64-logits64'}


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    dll = compile_for_host(tmp_path_factory.mktemp('host_heat_marginals'), 'host_heat_marginals', ['heat_marginals.hip'], HOST_BODY)
    dll.host_heat_marginals.restype = C.c_int
    dll.host_heat_marginals.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                        C.c_void_p]
    return dll


def case_permutation(j):
    """Non-identity, with a head joint left out and one repeated where there are several."""
    return [0] if j == 1 else list(range(j - 1, 0, -1)) + [j - 1]


def case_logits(side, j, d, n, precise):
    rng = np.random.default_rng([side, j, d, n])
    gain = (1.0, 8.0)[(side + j + n) % 2]
    lg = rng.standard_normal((n, side, side, d * j)) * gain + rng.uniform(-30, 30)
    return np.ascontiguousarray(lg.astype(np.float64 if precise == 2 else np.float32))


def run_host(dll, lg, j, d, perm, precise):
    n, side = lg.shape[:2]
    xy, z = np.full((n, len(perm), side, side), np.nan, np.float32), np.full((n, len(perm), d), np.nan, np.float32)
    pa = np.asarray(perm, np.int32)
    tiles = dll.host_heat_marginals(lg.ctypes.data, precise, n, side, j, d, pa.ctypes.data, len(perm), xy.ctypes.data, z.ctypes.data)
    assert tiles == -(-side * side // (64 if side * side > 2048 else 32))
    return xy, z


def host_deviations(dll):
    """{key: (abs, rel)}: the worst figures of every host comparison of this file (tools/heat_marginals_parity.py records them)."""
    out = {}
    for precise, key in ACC_KEYS.items():
        worst = [0.0, 0.0]
        for side, j, d, n in HOST_CASES:
            lg, perm = case_logits(side, j, d, n, precise), case_permutation(j)
            xy, z = run_host(dll, lg, j, d, perm, precise)
            rxy, rz = HR.marginals(lg, j, d, perm)
            for got, ref in ((xy, rxy), (z, rz)):
                a, r = HR.deviation(got, ref)
                worst = [max(worst[0], a), max(worst[1], r)]
        out[key] = tuple(worst)
    return out


@pytest.mark.parametrize('precise', (0, 1, 2))
@pytest.mark.parametrize('side,j,d,n', HOST_CASES, ids=lambda v: str(v))
def test_host_compiled_kernel_code_against_the_restatement(host, side, j, d, n, precise):
    lg, perm = case_logits(side, j, d, n, precise), case_permutation(j)
    xy, z = run_host(host, lg, j, d, perm, precise)
    rxy, rz = HR.marginals(lg, j, d, perm)
    HR.check(xy, z, rxy, rz, ACC_KEYS[precise], min(s * s * dd for s in SIDES for _, dd in HEADS), f'S{side} J{j} D{d} n{n}')
    assert np.allclose(xy.astype(np.float64).sum((2, 3)), 1, atol=1e-5) and np.allclose(z.astype(np.float64).sum(2), 1, atol=1e-5)


@pytest.mark.parametrize('precise', (0, 1, 2))
def test_host_compiled_code_on_the_known_answers(host, precise):
    """Shift invariance (the maximum is subtracted), the delta, -Inf voxels, and NaN / +Inf confined to their joint."""
    dt = np.float64 if precise == 2 else np.float32
    side, j, d = 7, 3, 4                     # 49 pixels: two tiles, the second ragged
    rng = np.random.default_rng(11)
    lg = (rng.standard_normal((2, side, side, d * j)) * 2).astype(dt)
    perm = [2, 0, 1]
    xy, z = run_host(host, lg, j, d, perm, precise)
    for shift in (80.0, -80.0):
        sxy, sz = run_host(host, (lg + dt(shift)).astype(dt), j, d, perm, precise)
        rxy, rz = HR.marginals((lg + dt(shift)).astype(dt), j, d, perm)
        HR.check(sxy, sz, rxy, rz, ACC_KEYS[precise], 2 * 2 * 4, f'shift {shift:+g}')
    spike = lg.copy()
    spike[0, 6, 5, 3 * j + 1] = 60.0                                      # in the ragged tile
    spike[1, :3, :, 0 * j + 0] = -np.inf                                  # voxels of weight zero
    sxy, sz = run_host(host, spike, j, d, perm, precise)
    assert sxy[0, 2, 6, 5] == 1 and sz[0, 2, 3] == 1 and sxy[0, 2].sum() == 1 and sz[0, 2].sum() == 1
    rxy, rz = HR.marginals(spike, j, d, perm)
    assert np.isfinite(sxy).all() and (sxy[1, 1, :3] <= rxy[1, 1, :3].max() * 1.001).all()
    HR.check(sxy, sz, rxy, rz, ACC_KEYS[precise], 2 * 2 * 4, 'spike and -Inf')
    for bad in (np.nan, np.inf):
        poisoned = lg.copy()
        poisoned[1, 3, 3, 2 * j + 0] = bad
        pxy, pz = run_host(host, poisoned, j, d, perm, precise)
        assert np.isnan(pxy[1, 1]).all() and np.isnan(pz[1, 1]).all(), bad
        keep = np.ones((2, 3), bool)
        keep[1, 1] = False
        assert np.array_equal(pxy[keep], xy[keep]) and np.array_equal(pz[keep], z[keep]), bad


def test_recorded_tolerances_are_the_figures_of_this_code(host):
    """The file the gates come from holds what the host comparisons give (same compiler, same libm: to 1 %), so a gate can
    only have come from a measurement; and every gate is below one voxel of the smallest head."""
    rec = HR.recorded()
    for key, (a, r) in host_deviations(host).items():
        w = rec['worst'][key]
        print(f'heat_marginals {key}: abs {a:.3e} (recorded {w["abs"]:.3e}) rel {r:.3e} (recorded {w["rel"]:.3e})')
        assert a <= w['abs'] * 1.01 and r <= w['rel'] * 1.01, (key, a, r, w)
    for key in rec['worst']:
        HR.gate(key, rec['smallest_voxels'][key])


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------

def test_new_symbols_in_header_bindings_and_library(lib):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'metro_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(metro_[a-z0-9_]+)\s*\(', text))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        params = re.search(r'\b' + name + r'\s*\(([^)]*)\)', text).group(1)
        assert len(_lib.SIGNATURES[name][1]) == params.count(',') + 1, name
        assert 'stream' not in params, name                    # binding is host state: no launching entry was added
    assert lib.metro_abi_version() == 8 == _lib.ABI_VERSION
    assert re.search(r'#define\s+METRO_ABI_VERSION\s+8\b', open(os.path.join(ROOT, 'include', 'metro_hip.h')).read())
    from metro_pose3d_amd import build
    assert 'heat_marginals.hip' in build.SOURCES


def test_c_refusals(lib):
    spec = ModelSpec(50, 16, 'h36m', base_width=16)
    plans = {}
    try:
        for prec in (_lib.METRO_PREC_F16, _lib.METRO_PREC_F64):
            plans[prec] = C.c_void_p()
            cs = spec.to_c(prec)
            assert lib.metro_plan_create(C.byref(cs), 4, C.byref(plans[prec])) == 0
        plan = plans[_lib.METRO_PREC_F16]
        side, c, nj = spec.heatmap_side, spec.n_head_channels, spec.skeleton.n_head
        up = lambda v: (v + 255) // 256 * 256
        tiles = side * side // 32
        records = lambda n: up(n * tiles * c * 2 * 8) + up(n * nj * 2 * 8)
        # the one-launch head keeps its logits on chip: the scratch also holds them as fp32; the parity plans read the workspace
        assert lib.metro_plan_heatmaps_scratch_bytes(plan, 3) == records(3) + up(3 * side * side * c * 4)
        assert lib.metro_plan_heatmaps_scratch_bytes(plans[_lib.METRO_PREC_F64], 3) == records(3)
        for bad in (0, -1, 5):
            assert lib.metro_plan_heatmaps_scratch_bytes(plan, bad) == -1
        assert lib.metro_plan_heatmaps_scratch_bytes(None, 1) == -1
        p = C.c_void_p(4096)
        assert lib.metro_plan_bind_heatmaps(None, p, p, p, 1) == -1
        for xy, z, scr in ((None, p, p), (p, None, p), (p, p, None), (None, None, p), (None, None, None)):
            assert lib.metro_plan_bind_heatmaps(plan, xy, z, scr, 2) == -1, (xy, z, scr)
            assert b'go together' in lib.metro_last_error()
        for bad in (0, -1, 5):
            assert lib.metro_plan_bind_heatmaps(plan, p, p, p, bad) == -1 and b'max_n' in lib.metro_last_error()
        assert lib.metro_plan_bind_heatmaps(plan, p, p, C.c_void_p(4100), 2) == -1 and b'aligned' in lib.metro_last_error()
        assert lib.metro_plan_bind_heatmaps(plan, None, None, None, 0) == 0            # unbinding what is not bound
        # a bound forward with n > max_n is refused before any launch (and before any pointer is read: these are not memory)
        assert lib.metro_plan_bind_params(plan, C.c_void_p(4096)) == 0
        assert lib.metro_plan_bind_heatmaps(plan, p, p, p, 2) == 0
        assert lib.metro_kernel_notes(1) == 0
        assert lib.metro_forward(plan, p, 3, p, p, None) == -1 and b'bound heat-map buffers' in lib.metro_last_error()
        assert lib.metro_forward_coords01(plan, p, 3, p, p, p, None) == -1
        assert lib.metro_forward_u8(plan, p, 3, p, None, p, None) == -1
        assert lib.metro_forward_moments(plan, p, 0, 4, p, None, None, None, None, p, None) == -1
        assert lib.metro_last_kernel_id() == b''
        assert lib.metro_kernel_notes(0) == 0
        assert lib.metro_plan_bind_heatmaps(plan, None, None, None, 0) == 0
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
    names = list(inspect.signature(INF.estimate_pose).parameters)
    assert names[-2:] == ['return_uncertainty', 'return_heatmaps']
    assert inspect.signature(INF.estimate_pose).parameters['return_heatmaps'].default is False
    names = list(inspect.signature(Engine.forward).parameters)
    assert names[-2:] == ['heat_xy', 'heat_z'] and names[:6] == ['self', 'images', 'out', 'coords01', 'cov01', 'peak']
    assert all(inspect.signature(Engine.forward).parameters[k].default is None for k in ('heat_xy', 'heat_z'))
    assert 'Heatmaps' in M.__all__ and M.Heatmaps is INF.Heatmaps and INF.Heatmaps._fields == ('xy', 'z')
    with pytest.raises(SystemExit):
        INF.main(['--heatmaps', 'out.npz'])                # --model-path is still required: argparse exits, not "unknown flag"
    spec = ModelSpec(50, 16, 'h36m', depth=4)
    eng = Engine(spec, None, 'f16', max_batch=4)
    eng._blob, eng.device = object(), torch.device('cpu')          # past the "no parameters" check, never launched
    nj, side = spec.skeleton.n_out, spec.heatmap_side
    assert eng.heat_shapes(2) == ((2, nj, side, side), (2, nj, 4))
    x = torch.zeros((2, 256, 256, 3))
    xy, z = torch.zeros((2, nj, side, side)), torch.zeros((2, nj, 4))
    with pytest.raises(ValueError, match='go together'):
        eng.forward(x, heat_xy=xy)
    with pytest.raises(ValueError, match='go together'):
        eng.forward(x, heat_z=z)
    with pytest.raises(ValueError, match='heat_xy must be'):
        eng.forward(x, heat_xy=xy[:, :, :-1], heat_z=z)
    with pytest.raises(ValueError, match='heat_xy must be'):
        eng.forward(x, heat_xy=xy[:1], heat_z=z)
    with pytest.raises(ValueError, match='heat_z must be'):
        eng.forward(x, heat_xy=xy, heat_z=z.double())
    with pytest.raises(ValueError, match='heat_z must be'):
        eng.forward(x, heat_xy=xy, heat_z=torch.zeros((2, nj, 8)))
    with pytest.raises(ValueError, match='heat_xy must be'):
        eng.forward(x, heat_xy=xy.numpy(), heat_z=z)
    eng.heat_chunk = 3
    assert eng._heat_chunk() == 3
    eng.heat_chunk = None
    assert eng._heat_chunk() == 4
    eng._blob = None
    eng.close()
