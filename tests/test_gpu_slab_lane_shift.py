"""conv3x3_f16_slab's lane-shift form (slab_tile: HS) against fp64, through metro_conv_f16: on maps and sub-images 16 pixels wide the
side taps of a kernel row are the centre tap's fragment shifted by lanes instead of read from LDS (tests/test_slab_lane_shift_algebra.py
holds the identity).  The form is another implementation of the same instantiation, so the kernel id does not name it; what holds it
is the result.

Exact cases: operands are small integers, so every summation order gives the exact fp16 result and the output must equal the fp64
reference BIT FOR BIT.  Inputs are in {0, 1}; columns 0, d - 1, 16 - d and 15 (the ones a shift by d moves padding into or out of) carry
their own value, 2 .. 5, on every eighth channel and zero elsewhere; weights are in {-1, 0, 1}, the bias is a small integer.  A tap of a
pixel then adds at most c_in in magnitude (c_in ones, or c_in / 8 fives), so |sum| <= 9 * 128 + 8 < 2048: exact in fp32 and in fp16.
Gaussian cases: the same shapes with the conv contract's operands, within 2e-3 of the layer maximum.
Non-finite cases: one NaN / one Inf at an edge column poisons exactly the outputs whose in-image taps reach it (0 * NaN and 0 * Inf are
NaN, whatever the weight); everything else keeps the clean run's bits -- where the plain form puts them.

Widths 8 and 32 are guards: the identity fails there, the launcher must keep the plain reads, and a shift taken by mistake is a wrong
result in the exact cases."""
import ctypes as C
import zlib
from dataclasses import dataclass

import numpy as np
import pytest
import torch

from metro_pose3d_amd._lib import check
from tests import helpers as H

pytestmark = pytest.mark.gpu

B1, T3, T128 = '64x256,rows320,bufs1,tps1,kc64,ws3>', '64x256,rows320,bufs2,tps3,kc64,ws3>', '128x256,rows320,bufs2,tps1,kc64,ws3>'


@dataclass
class Case:
    name: str
    tile: str          # the id is conv3x3_f16_slab< + this
    n: int             # images launched
    h: int
    w: int
    c_in: int
    c_out: int
    rate: int
    period: int = 0    # > 0: the images repeat with this period; the reference is computed for one period

    @property
    def distinct(self):
        return self.period or self.n

    @property
    def shift(self):
        """The horizontal tap distance inside the (sub-)image the kernel walks: the columns a shift would touch."""
        return 1 if self.tile.endswith('+subgrid') else self.rate

    def desc(self, n=None):
        return H.conv_desc(self.n if n is None else n, self.h, self.c_in, self.h, self.c_out, 3, 1, self.rate, self.rate,
                           w_in=self.w, w_out=self.w)


CASES = [
    Case('one_tile_single_chunk', B1, 1, 16, 16, 64, 64, 1),
    Case('tps3_two_chunks', T3, 2, 16, 16, 128, 64, 1),
    Case('tps3_rate2_halo32', T3, 3, 16, 16, 128, 64, 2),
    Case('tps3_16x8_ragged_tiles', T3, 3, 8, 16, 128, 64, 1),             # 384 pixels: tiles cross images, ragged last tile
    Case('cout128_rate2', T128, 256, 16, 16, 64, 128, 2, period=4),        # the 128-cout tile needs 256 tiles
    Case('cout128_two_chunks', T128, 256, 16, 16, 128, 128, 1, period=4),  # ... and its not-last-chunk steps need c_in > 64
    Case('subgrid_64x64_rate4', B1 + '+subgrid', 1, 64, 64, 64, 64, 4),    # 16-wide sub-images
    Case('guard_width8', T3, 4, 8, 8, 128, 64, 1),
    Case('guard_width32', T3, 1, 32, 32, 128, 64, 1),
]
IDS = [c.name for c in CASES]


def _rng(*parts):
    return np.random.default_rng(zlib.crc32('/'.join(map(str, parts)).encode()))


def _edge_columns(case):
    """Columns 0, d - 1, 16 - d and 15 of the 16-wide (sub-)image; on the guards' maps also the map's own last columns."""
    d = case.shift
    gw = case.w // case.rate if case.tile.endswith('+subgrid') else case.w
    return sorted({c for c in (0, d - 1, 16 - d, 15, gw - d, gw - 1) if c < gw})


def _integer_operands(case):
    rng = _rng('slab_lane_shift', 'int', case.name)
    x = rng.integers(0, 2, (case.distinct, case.h, case.w, case.c_in)).astype(np.float64)
    step = case.rate if case.tile.endswith('+subgrid') else 1            # column c of a sub-image is column c * rate + sx of the map
    for i, col in enumerate(_edge_columns(case)):
        for sx in range(step):
            x[:, :, col * step + sx, :] = 0.0
            x[:, :, col * step + sx, i % 8::8] = 2.0 + i
    w = rng.integers(-1, 2, (case.c_out, 3, 3, case.c_in)).astype(np.float64)
    b = rng.integers(-8, 9, case.c_out).astype(np.float64)
    return x, w, b


def _gauss_operands(case):
    rng = _rng('slab_lane_shift', 'gauss', case.name)
    x = rng.standard_normal((case.distinct, case.h, case.w, case.c_in))
    w = rng.standard_normal((case.c_out, 3, 3, case.c_in)) * np.sqrt(2.0 / (9 * case.c_in))
    b = rng.standard_normal(case.c_out) * 0.1
    return x, w, b


def _run(lib, cuda, case, x16, w16, b32):
    """Launches the layer on the case's n images (x16 holds one period) and returns the output [n, h, w, c_out] as float16."""
    reps = case.n // x16.shape[0]
    tx = torch.from_numpy(x16).to(cuda).repeat(reps, 1, 1, 1).contiguous()
    tw, tb = torch.from_numpy(w16).to(cuda), torch.from_numpy(b32).to(cuda)
    out = torch.full((case.n, case.h, case.w, case.c_out), float('nan'), dtype=torch.float16, device=cuda)
    d = case.desc()
    check(lib.metro_kernel_notes(1), 'metro_kernel_notes')
    try:
        check(lib.metro_conv_f16(C.byref(d), H.ptr(tx), H.ptr(tw), H.ptr(tb), None, None, None, H.ptr(out), None),
              f'metro_conv_f16 {case.name}')
        torch.cuda.synchronize()
        kid = lib.metro_last_kernel_id().decode()
    finally:
        lib.metro_kernel_notes(0)
    assert kid == 'conv3x3_f16_slab<' + case.tile, (case.name, kid)
    return out.cpu().numpy()


def _reference(case, x16, w16, b32):
    y, _ = H.ref_conv_desc(case.desc(case.distinct), x16, w16, b32)
    return y


def _twins_hold_the_same_bits(case, got):
    """Every image of a periodic batch holds the bits of its twin in the first period; returns the first period."""
    p = case.distinct
    g = got.view(np.uint16).reshape(case.n // p, p, *got.shape[1:])
    assert (g == g[:1]).all(), f'{case.name}: {int((g != g[:1]).any(axis=(1, 2, 3, 4)).sum())} periods differ from the first'
    return got[:p]


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_integer_operands_give_the_exact_result_bit_for_bit(lib, cuda, case):
    x, w, b = _integer_operands(case)
    x16, w16, b32 = x.astype(np.float16), w.astype(np.float16), b.astype(np.float32)
    y = _reference(case, x16, w16, b32)
    assert np.abs(y).max() < 2048 and (y == np.rint(y)).all()
    got = _twins_hold_the_same_bits(case, _run(lib, cuda, case, x16, w16, b32))
    want = y.astype(np.float16)
    bad = got.view(np.uint16) != want.view(np.uint16)
    assert not bad.any(), (f'{case.name}: {int(bad.sum())} of {bad.size} elements differ; first at {tuple(np.argwhere(bad)[0])}: '
                           f'got {got[bad][0]!r} want {want[bad][0]!r}; columns hit {sorted(set(np.argwhere(bad)[:, 2].tolist()))}')


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_gaussian_operands_within_the_contract_bound(lib, cuda, case):
    x, w, b = _gauss_operands(case)
    x16, w16, b32 = x.astype(np.float16), w.astype(np.float16), b.astype(np.float32)
    y = _reference(case, x16, w16, b32)
    got = _twins_hold_the_same_bits(case, _run(lib, cuda, case, x16, w16, b32)).astype(np.float64)
    assert np.isfinite(got).all()
    err, bound = np.abs(got - y).max(), 2e-3 * np.abs(y).max()
    print(f'{case.name}: max|err| {err:.3e}  bound {bound:.3e}')
    assert err <= bound, (case.name, err, bound)


NONFINITE = [c for c in CASES if c.name in ('tps3_rate2_halo32', 'one_tile_single_chunk', 'guard_width32')]


@pytest.mark.parametrize('value', [np.nan, np.inf], ids=['nan', 'inf'])
@pytest.mark.parametrize('case', NONFINITE, ids=[c.name for c in NONFINITE])
def test_a_nonfinite_input_at_an_edge_column_lands_where_the_plain_form_puts_it(lib, cuda, case, value):
    x, w, b = _integer_operands(case)
    x16, w16, b32 = x.astype(np.float16), w.astype(np.float16), b.astype(np.float32)
    clean = _reference(case, x16, w16, b32).astype(np.float16)
    r = case.rate
    img = case.n - 1
    for py, px, ch in ((0, case.w - 1, 5), (case.h - 1, 0, case.c_in - 3), (case.h // 2, r - 1, 17), (case.h // 2 + 1, case.w - r, 40)):
        xp = x16.copy()
        xp[img, py, px, ch] = value
        got = _run(lib, cuda, case, xp, w16, b32)
        # the outputs whose taps reach (py, px): (py - dr, px - ds) for the nine (dr, ds) in {-r, 0, r}^2 that stay inside the image
        hit = np.zeros(got.shape[:3], bool)
        for dr in (-r, 0, r):
            for ds in (-r, 0, r):
                if 0 <= py - dr < case.h and 0 <= px - ds < case.w:
                    hit[img, py - dr, px - ds] = True
        what = f'{case.name}: {value} at image {img} ({py}, {px}) channel {ch}'
        fin = np.isfinite(got)
        assert not fin[hit].any(), f'{what}: {int(fin[hit].sum())} reached outputs stayed finite'
        if np.isnan(value):
            assert np.isnan(got[hit]).all(), what
        assert fin[~hit].all(), f'{what}: non-finite outputs at {np.argwhere(~fin & ~hit[..., None])[:4].tolist()} are out of its reach'
        assert (got[~hit].view(np.uint16) == clean[~hit].view(np.uint16)).all(), f'{what}: an output out of its reach changed'
