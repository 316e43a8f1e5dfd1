"""csrc/camera_math.h without a GPU: the header compiled for the host, each function held bit for bit to a restatement that
performs one rounded operation per line -- NumPy scalars of the function's type, and exact rational arithmetic rounded once
for the fused multiply-adds."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from tests.helpers import compile_for_host
from tests.test_frames import FIX, fixture_cameras


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    dll = compile_for_host(tmp_path_factory.mktemp('host_camera_math'), 'host_camera_math', ['camera_math.h'], '''
extern "C" void host_distort_normalized(const float* d, const float* in, int n, float* out) {
    for (int i = 0; i < n; ++i) {
        float px = in[2 * i], py = in[2 * i + 1];
        metro::distort_normalized(d, px, py);
        out[2 * i] = px; out[2 * i + 1] = py;
    }
}
extern "C" void host_inv3(const double* a, double* o) { metro::inv3(a, o); }
extern "C" void host_mm3_rounded(const double* a, const double* b, double* o) { metro::mm3_rounded(a, b, o); }
extern "C" void host_mm3_gemm_f64(const double* a, const double* b, double* o) { metro::mm3_gemm<double>(a, b, o); }
''')
    for name, nargs in (('host_inv3', 2), ('host_mm3_rounded', 3), ('host_mm3_gemm_f64', 3)):
        getattr(dll, name).restype = None
        getattr(dll, name).argtypes = [C.c_void_p] * nargs
    dll.host_distort_normalized.restype = None
    dll.host_distort_normalized.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    return dll


def _call(fn, *mats):
    mats = [np.ascontiguousarray(m, np.float64).reshape(9) for m in mats]
    out = np.full(9, np.nan)
    fn(*[C.c_void_p(m.ctypes.data) for m in mats], C.c_void_p(out.ctypes.data))
    return out


def _matrices():
    """(K, R, K R) of the fixture cameras as fp64 arrays of 9: the matrices the kernels invert and multiply."""
    out = []
    for c in fixture_cameras(np.load(FIX)):
        k, r = np.asarray(c.intrinsic_matrix, np.float64), np.asarray(c.R, np.float64)
        out.append((k.reshape(9), r.reshape(9), (k @ r).reshape(9)))
    return out


# ---- distort_normalized ------------------------------------------------------------------------------------------------------

def distort_ref(d, px, py):
    """project_points' chain (reference cameralib.py:375-397) on np.float32 scalars, one rounded operation per line."""
    f = np.float32
    d = [f(v) for v in d]
    px, py = f(px), f(py)
    t0 = px * px
    t1 = py * py
    r2 = t0 + t1
    r4 = r2 * r2
    dist = d[0] * r2
    t = d[1] * r4
    dist = dist + t
    r6 = r4 * r2
    t = d[4] * r6
    dist = dist + t
    dist = dist + f(1)
    t = f(2) * d[3]
    t = px * t
    dist = dist + t
    t = f(2) * d[2]
    t = py * t
    dist = dist + t
    px = px * dist
    t = r2 * d[3]
    px = px + t
    py = py * dist
    t = r2 * d[2]
    py = py + t
    return px, py


def _coefficient_sets():
    sets = [('zero', np.zeros(5, np.float32))]
    for i, c in enumerate(fixture_cameras(np.load(FIX))):
        if c.distortion_coeffs is not None:
            sets.append((f'camera {i}', np.asarray(c.distortion_coeffs, np.float32)))
    assert len(sets) >= 3                     # the fixture has two distorted cameras
    return sets


def _points():
    rng = np.random.default_rng(7)
    grid = np.stack(np.meshgrid(np.linspace(-1.5, 1.5, 13), np.linspace(-1.2, 1.2, 11)), -1).reshape(-1, 2)
    pts = np.concatenate([grid, rng.normal(0, 0.6, (200, 2)), [[0.0, 0.0], [-0.0, 1e-30]],
                          [[3e6, 1.0], [-2e7, 4e6], [1e13, -1e13]],                # r2 > 7e12: r4 r2 overflows fp32 (and r2 itself)
                          [[np.nan, 0.25], [0.25, np.nan], [np.inf, 0.0]]]).astype(np.float32)
    with np.errstate(all='ignore'):
        r2 = pts[:, 0] * pts[:, 0] + pts[:, 1] * pts[:, 1]
        assert np.isinf((r2 * r2) * r2).sum() >= 3 and np.isnan(pts).any()
    return pts


@pytest.mark.parametrize('name,d', _coefficient_sets(), ids=[n for n, _ in _coefficient_sets()])
def test_distort_normalized_matches_the_float32_restatement_bit_for_bit(host, name, d):
    pts = _points()
    got = np.full_like(pts, 7.0)
    d = np.ascontiguousarray(d, np.float32)
    host.host_distort_normalized(C.c_void_p(d.ctypes.data), C.c_void_p(pts.ctypes.data), len(pts), C.c_void_p(got.ctypes.data))
    with np.errstate(all='ignore'):
        want = np.array([distort_ref(d, x, y) for x, y in pts], np.float32)
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))       # NaN payloads: both NaN
    assert same.all(), (name, pts[~same.all(axis=1)][:4], got[~same.all(axis=1)][:4], want[~same.all(axis=1)][:4])
    if name == 'zero':                         # no coefficients: dist = 1, the point unchanged wherever r6 is finite
        fin = np.isfinite(pts).all(axis=1) & (np.abs(pts).max(axis=1) < 10)
        assert np.array_equal(got[fin], pts[fin])


# ---- inv3, mm3_rounded ---------------------------------------------------------------------------------------------------------

def inv3_ref(a):
    """The adjugate over the determinant on np.float64 scalars, one rounded operation per line."""
    a = [np.float64(v) for v in a]

    def cof(p, q, r, s):                       # a[p] a[q] - a[r] a[s]
        t0 = a[p] * a[q]
        t1 = a[r] * a[s]
        return t0 - t1

    c00, c01, c02 = cof(4, 8, 5, 7), cof(5, 6, 3, 8), cof(3, 7, 4, 6)
    t0 = a[0] * c00
    t1 = a[1] * c01
    t2 = a[2] * c02
    det = t0 + t1
    det = det + t2
    num = [c00, cof(2, 7, 1, 8), cof(1, 5, 2, 4), c01, cof(0, 8, 2, 6), cof(2, 3, 0, 5), c02, cof(1, 6, 0, 7), cof(0, 4, 1, 3)]
    return np.array([n / det for n in num], np.float64)


def mm3_rounded_ref(a, b):
    a, b = [np.float64(v) for v in a], [np.float64(v) for v in b]
    o = np.empty(9)
    for i in range(3):
        for j in range(3):
            t0 = a[i * 3 + 0] * b[0 * 3 + j]
            t1 = a[i * 3 + 1] * b[1 * 3 + j]
            t2 = a[i * 3 + 2] * b[2 * 3 + j]
            s = t0 + t1
            o[i * 3 + j] = s + t2
    return o


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def test_inv3_and_mm3_rounded_match_the_float64_restatement_bit_for_bit(host):
    for k, r, kr in _matrices():
        for m in (k, kr):
            got = _call(host.host_inv3, m)
            assert np.array_equal(_bits(got), _bits(inv3_ref(m)))
            assert np.allclose((got.reshape(3, 3) @ m.reshape(3, 3)), np.eye(3), rtol=0, atol=1e-9)      # and it is the inverse
        inv_kr = inv3_ref(kr)
        for a, b in ((k, r), (kr, inv_kr), (inv_kr, k)):
            assert np.array_equal(_bits(_call(host.host_mm3_rounded, a, b)), _bits(mm3_rounded_ref(a, b)))


# ---- mm3_gemm<double> ----------------------------------------------------------------------------------------------------------

def fma_exact(a, b, c):
    """fma(a, b, c): the exact a b + c rounded once (float(Fraction) rounds correctly)."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def mm3_gemm_ref(a, b):
    a, b = [float(v) for v in a], [float(v) for v in b]
    o = np.empty(9)
    for i in range(3):
        for j in range(3):
            t = a[i * 3 + 0] * b[j]                                    # the first product is rounded
            t = fma_exact(a[i * 3 + 1], b[3 + j], t)
            o[i * 3 + j] = fma_exact(a[i * 3 + 2], b[6 + j], t)
    return o


def test_mm3_gemm_double_matches_the_exact_fma_restatement_bit_for_bit(host):
    differs = 0
    for k, r, kr in _matrices():
        inv_kr = inv3_ref(kr)
        for a, b in ((k, r), (kr, inv_kr), (inv_kr, k)):
            got = _call(host.host_mm3_gemm_f64, a, b)
            assert np.array_equal(_bits(got), _bits(mm3_gemm_ref(a, b)))
            differs += int((_bits(got) != _bits(mm3_rounded_ref(a, b))).sum())
    assert differs > 0                         # the cases tell the fused chain from the every-product-rounded one


def test_the_build_knows_the_header_and_the_split_source():
    from metro_pose3d_amd import build
    assert 'camera_math.h' in build.HEADERS              # an edit to the header makes every object stale
    assert 'warp_crops.hip' in build.SOURCES and 'pool_softargmax.hip' in build.SOURCES
