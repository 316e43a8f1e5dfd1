"""The three heat-map kernel families (csrc/heat_marginals.hip, heat_modes.hip, heat_posterior.hip) on the MI355X on volumes
chosen to break them, through the kernel-level entries metro_heat_marginals, metro_heat_modes and metro_heat_posterior: every
case is held to the fp64 restatement of its kernel (tests/heat_*_ref.py) for precise 0 (fp32 logits, fp32 sums), 1 (fp32 logits,
fp64 sums) and 2 (fp64 logits).  MetroSpec is filled through ctypes (proc_side = 32 S, stride 32), so any side is reachable.

  a  the crafted lists of the host tests (tests/test_heat_modes.py, test_heat_posterior.py, test_heat_marginals.py) on the device:
     there they run on a team of one thread, here on the workgroup
  b  modes: inputs chosen by who owns a voxel in the selection scan (thread (v / 4) % 256, wave = thread / 64), by window size,
     by slab seam, by flag tail and by one bad voxel.  The ownership formula only picks inputs: the expectation is always the
     restatement, and every case states on the restatement alone the property it is there for (`claim`;
     tests/test_heat_volumes.py runs the claims without a GPU)
  c  posterior: on either side of the LDS staging decision, S = 1, 131 072 voxels, and extreme priors
  d  marginals: on either side of the tile width, ragged tiles, C > 256, chunk < tile, -Inf channels and joints
  e  bits: a crop's position in the call, two output rows of one head joint, sentinels around the outputs, and the bound
     forward's outputs against the entries on the dumped logits of the same forward

The case lists are module-level data, importable without a GPU: tests/test_heat_volumes.py closes them over the shape classes
the supported grid reaches (modes_class, posterior_class, marginals_class below mirror md_slab_rows, po_fits, hm_tile_pixels and
hm_chunk_pixels; that file holds the mirrors to the kernel files' own helpers compiled for the host).

Tolerances: the keys gpu/acc32-logits32, gpu/acc64-logits32 and gpu/acc64-logits64 of profiles/heat_*_parity.json hold the worst
deviation of each kernel from the restatement over the cases of this file (tools/heat_*_parity.py run gpu_deviations() below);
the tests assert the files' standing gate, four times that figure.  On the cases shared with the host lists the two fp64-sum
figures may not exceed twice the host's recorded ones (modes, marginals: both are fp64 sums rounded once to fp32); the
posterior's host figures are recorded BEFORE that rounding (1e-12), so there the bar is twice the deviation of the restatement's
own rounding to fp32."""
import ctypes as C
import functools
from typing import Callable, NamedTuple, Tuple

import numpy as np
import pytest
import torch

from metro_pose3d_amd import _lib
from metro_pose3d_amd._lib import check
from tests import heat_marginals_ref as HR, heat_modes_ref as MR, heat_posterior_ref as PR
from tests import test_heat_marginals as TH, test_heat_modes as TM, test_heat_posterior as TP

pytestmark = pytest.mark.gpu

PRECISES = (0, 1, 2)
KEYS = {0: 'gpu/acc32-logits32', 1: 'gpu/acc64-logits32', 2: 'gpu/acc64-logits64'}
HOST_KEYS = {1: 'host/acc64-logits32', 2: 'host/acc64-logits64'}
PAD = 256                       # sentinel words in front of and behind every output
SENTINEL = -7.0


# ---- the shape decisions of the three launchers, restated (held to the kernel files' own helpers in tests/test_heat_volumes.py) ----

def slab_rows(side, depth, logit_bytes):
    """md_slab_rows: y-rows of a slab besides its halo rows; `side` when the volume is staged whole; 0 when it is refused."""
    avail = 64 * 1024 - 128 - ((side * side * depth + 15) & ~15)
    if avail <= 0:
        return 0
    fit = avail // (side * depth * logit_bytes)
    return side if fit >= side else fit - 2 if fit >= 3 else 0


def modes_class(side, depth, precise):
    rows = slab_rows(side, depth, 8 if precise == 2 else 4)
    return ('refused',) if rows == 0 else ('whole',) if rows >= side else ('slabs', 'ragged' if side % rows else 'even')


def posterior_class(side, depth, precise):
    return ('staged',) if side * side * depth * (8 if precise == 2 else 4) + 256 <= 64 * 1024 else ('streamed',)


def tile_pixels(pixels):
    return 64 if pixels > 2048 else 32


def chunk_pixels(pixels, channels, acc_bytes):
    return max(1, min(32768 // (channels * acc_bytes), tile_pixels(pixels)))


def marginals_class(side, joints, depth, precise):
    pixels, c = side * side, depth * joints
    tile = tile_pixels(pixels)
    return (f'tile{tile}', 'ragged' if pixels % tile else 'even', 'C>256' if c > 256 else 'C<=256',
            'chunk<tile' if chunk_pixels(pixels, c, 4 if precise == 0 else 8) < tile else 'chunk=tile')


# ---- cases ---------------------------------------------------------------------------------------------------------------------

def fp32_values(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def repeat_last(j):
    """Every head joint in order, the last one twice: two output rows of one head joint."""
    return list(range(j)) + [j - 1]


def vol5(lg, d, j):
    """[n, S, S, D*J] -> the view [n, y, x, d, j]."""
    return lg.reshape(lg.shape[0], lg.shape[1], lg.shape[2], d, j)


def lin(v, side, d):
    return v // (side * d), v // d % side, v % d


def owner(v):
    """(thread, wave, lane) of the workgroup member whose flag words hold voxel v in the selection scan of modes_walk."""
    t = (v // 4) % 256
    return t, t // 64, t % 64


def window_extents(v, side, d, radius):
    return tuple(min(c + radius, k - 1) - max(c - radius, 0) + 1 for c, k in zip(lin(int(v), side, d), (side, side, d)))


def window_count(v, side, d, radius):
    return int(np.prod(window_extents(v, side, d, radius)))


class ModesCase(NamedTuple):
    name: str
    side: int
    d: int
    j: int
    n: int
    k: int
    radius: int
    precises: Tuple[int, ...]
    build: Callable            # (logit_bytes) -> logits fp64 [n, S, S, D*J], fp32 values
    claim: Callable            # (case, logits, ref voxel, ref stats, logit_bytes): asserts what the case is there for

    @property
    def perm(self):
        return repeat_last(self.j)


# -- ties across waves and lanes: eight strict peaks of one logit, owned as the docstring of the module says
TIE_SIDE, TIE_D, TIE_LEVEL = 24, 8, 4.0
TIE_PEAKS = (803, 1827, 2563, 2700, 3331, 3500, 4099, 4340)


def build_ties(_bytes):
    rng = np.random.default_rng(41)
    lg = fp32_values(rng.standard_normal((2, TIE_SIDE, TIE_SIDE, TIE_D * 2)) * 0.5 - 2.0)
    for v in TIE_PEAKS:
        y, x, dd = lin(v, TIE_SIDE, TIE_D)
        vol5(lg, TIE_D, 2)[1, y, x, dd, 1] = TIE_LEVEL
    return lg


def claim_ties(case, lg, rv, rs, _bytes):
    vals = {float(vol5(lg, case.d, 2)[1][lin(v, case.side, case.d) + (1,)]) for v in TIE_PEAKS}
    assert vals == {TIE_LEVEL} and (vol5(lg, case.d, 2)[1, ..., 1] == TIE_LEVEL).sum() == 8           # one bit pattern, eight voxels
    assert rv[1, 1].tolist() == sorted(TIE_PEAKS) == list(TIE_PEAKS)                                   # selected by ascending index
    assert np.array_equal(rv[1, 2], rv[1, 1])
    waves = [owner(v)[1] for v in TIE_PEAKS]
    assert set(waves) == {0, 1, 2, 3} and waves == sorted(waves, reverse=True), waves                  # ascending v: descending waves
    same = [(a, b) for a in TIE_PEAKS for b in TIE_PEAKS if a < b and owner(a)[0] == owner(b)[0]]
    assert same == [(803, 1827)] and same[0][1] - same[0][0] == 1024                                   # one thread must offer two


# -- fewer candidates than k: joints of 0, 1, 5 and 8 candidates at k = 8
FEW_SPIKES = ((3, 3, 3), (3, 9, 4), (6, 6, 2), (9, 3, 5), (9, 9, 3), (6, 0, 6), (11, 11, 7))
FEW_COUNTS = (0, 1, 5, 8)


def build_few(_bytes):
    side, d, j = 12, 8, 4
    y, x, z = np.meshgrid(np.arange(side), np.arange(side), np.arange(d), indexing='ij')
    ramp = -(y + x + z) * 0.25                                  # one candidate: the origin
    lg = np.empty((2, side, side, d * j))
    v = vol5(lg, d, j)
    for i in range(2):
        v[i, ..., 0] = -np.inf
        for jj, spikes in ((1, 0), (2, 4), (3, 7)):
            v[i, ..., jj] = ramp - i
            for (sy, sx, sz) in FEW_SPIKES[:spikes]:
                v[i, sy, sx, sz, jj] += 5.0
    return fp32_values(lg)


def claim_few(case, lg, rv, rs, _bytes):
    assert case.k == 8
    for i in range(case.n):
        assert [(rv[i, r] >= 0).sum() for r in range(case.j)] == list(FEW_COUNTS)
        assert (rs[i, 0, :, 0] == 0).all() and np.isnan(rs[i, 0, :, 1:]).all()
    assert {owner((y * case.side + x) * case.d + z)[1] for y, x, z in FEW_SPIKES} == {0, 1, 2, 3}


# -- windows: one peak in the interior and one in each of the eight corners, at R = 0, 1 and 3; D = 1; S = 2
WIN_SIDE, WIN_D = 12, 8
WIN_PEAKS = ((5, 6, 4),) + tuple((y, x, z) for y in (0, WIN_SIDE - 1) for x in (0, WIN_SIDE - 1) for z in (0, WIN_D - 1))


def build_windows(_bytes):
    rng = np.random.default_rng(43)
    lg = fp32_values(rng.standard_normal((1, WIN_SIDE, WIN_SIDE, WIN_D * len(WIN_PEAKS))))
    for jj, (y, x, z) in enumerate(WIN_PEAKS):
        vol5(lg, WIN_D, len(WIN_PEAKS))[0, y, x, z, jj] = 8.0
    return lg


def claim_windows(case, lg, rv, rs, _bytes):
    first = rv[0, :len(WIN_PEAKS), 0]
    assert [lin(v, case.side, case.d) for v in first] == list(WIN_PEAKS)
    counts = [window_count(v, case.side, case.d, case.radius) for v in first]
    assert counts == {0: [1] * 9, 1: [27] + [8] * 8, 3: [343] + [64] * 8}[case.radius], counts


def build_small(side, d, j, seed):
    def build(_bytes):
        return fp32_values(np.random.default_rng(seed).standard_normal((2, side, side, d * j)) * 2)
    return build


def claim_clipped(case, lg, rv, rs, _bytes):
    """The clipping eats the window: an axis of one point (D = 1) or of two (S = 2) lies in it whole, whatever the radius."""
    assert (rv[..., 0] >= 0).all() and case.radius == 3
    for v in rv[rv >= 0]:
        ey, ex, ed = window_extents(v, case.side, case.d, case.radius)
        assert (ey, ex) == (2, 2) if case.side == 2 else (ed == 1 and case.d == 1 and max(ey, ex) <= case.side < 7)
        assert ey * ex * ed == window_count(v, case.side, case.d, case.radius) < 343


# -- slab seams: the launcher's slab height decides the rows
SEAM_D, SEAM_J = 8, 4
SEAM_PEAK, SEAM_LOWER = 4.0, 3.0


def seam_rows(side, logit_bytes):
    """The first rows of two slabs: the one in the middle of the volume and the last one (ragged where side % rows != 0)."""
    rows = slab_rows(side, SEAM_D, logit_bytes)
    assert 0 < rows < side, (side, logit_bytes, rows)
    seams = list(range(rows, side, rows))
    return rows, sorted({seams[len(seams) // 2], seams[-1]})


def seam_layout(side, logit_bytes):
    """-> (peaks, decoys) per joint: voxels (y, x, d) at SEAM_PEAK that are candidates, voxels that are not (a lower strict peak
    under a higher neighbour across the seam, or the later voxels of a plateau)."""
    _, seams = seam_rows(side, logit_bytes)
    peaks, decoys = [[] for _ in range(SEAM_J)], [[] for _ in range(SEAM_J)]
    for n_seam, s in enumerate(seams):
        x = 8 + 24 * n_seam
        peaks[0].append((s, x + 1, 3)); decoys[0].append((s - 1, x, 3))             # the last row of a slab under the next slab's first
        peaks[1].append((s - 1, x - 1, 4)); decoys[1].append((s, x, 4))             # the mirror image
        plateau = [(s - 1, x, 2), (s - 1, x + 1, 2), (s, x, 2), (s, x + 1, 2)]      # two rows high across the seam
        peaks[2].append(plateau[0]); decoys[2].extend(plateau[1:])
    peaks[3] = [(0, 5, 1), (side - 1, side - 6, 6)]                                 # the volume's first and last row
    return peaks, decoys


def build_seams(side):
    def build(logit_bytes):
        rng = np.random.default_rng([47, side])
        lg = fp32_values(rng.standard_normal((1, side, side, SEAM_D * SEAM_J)) * 0.3)
        peaks, decoys = seam_layout(side, logit_bytes)
        v = vol5(lg, SEAM_D, SEAM_J)
        for jj in range(SEAM_J):
            for at in peaks[jj]:
                v[(0,) + at + (jj,)] = SEAM_PEAK
            for at in decoys[jj]:
                v[(0,) + at + (jj,)] = SEAM_PEAK if jj == 2 else SEAM_LOWER
        return lg
    return build


def claim_seams(case, lg, rv, rs, logit_bytes):
    rows, seams = seam_rows(case.side, logit_bytes)
    assert modes_class(case.side, case.d, 2 if logit_bytes == 8 else 0)[0] == 'slabs' and case.radius == 0
    peaks, decoys = seam_layout(case.side, logit_bytes)
    index = lambda at: (at[0] * case.side + at[1]) * case.d + at[2]
    v = vol5(lg, case.d, case.j)
    for jj in range(case.j):
        want = sorted(index(at) for at in peaks[jj])
        assert len(want) < case.k and rv[0, jj, :len(want)].tolist() == want, (jj, rv[0, jj], want)
        rest = rv[0, jj, len(want):]
        assert (rest >= 0).all() and not set(rest.tolist()) & {index(at) for at in decoys[jj]}
        # every decoy is above the background the remaining modes come from: a false flag would have been selected
        assert all(v[(0,) + lin(u, case.side, case.d) + (jj,)] < SEAM_LOWER - 1 for u in rest)
        assert jj == 3 or all(any(at[0] in (s - 1, s) for s in seams) for at in peaks[jj] + decoys[jj])
    assert [at[0] for at in peaks[3]] == [0, case.side - 1]


# -- the flag tail: a volume that is no multiple of 4 voxels, a candidate in its last voxel
def build_tail(side, d):
    def build(_bytes):
        lg = fp32_values(np.random.default_rng([53, side, d]).standard_normal((2, side, side, d * 3)))
        vol5(lg, d, 3)[:, side - 1, side - 1, d - 1, :] = 5.0
        return lg
    return build


def claim_tail(case, lg, rv, rs, _bytes):
    vol = case.side * case.side * case.d
    assert vol % 4 and vol % 16 and (rv[..., 0] == vol - 1).all()


MODES_CASES = [
    ModesCase('ties', TIE_SIDE, TIE_D, 2, 2, 8, 1, PRECISES, build_ties, claim_ties),
    ModesCase('few-candidates', 12, 8, 4, 2, 8, 1, PRECISES, build_few, claim_few),
    ModesCase('windows-R0', WIN_SIDE, WIN_D, len(WIN_PEAKS), 1, 2, 0, PRECISES, build_windows, claim_windows),
    ModesCase('windows-R1', WIN_SIDE, WIN_D, len(WIN_PEAKS), 1, 2, 1, PRECISES, build_windows, claim_windows),
    ModesCase('windows-R3', WIN_SIDE, WIN_D, len(WIN_PEAKS), 1, 2, 3, PRECISES, build_windows, claim_windows),
    ModesCase('windows-D1', 5, 1, 2, 2, 2, 3, PRECISES, build_small(5, 1, 2, 44), claim_clipped),
    ModesCase('windows-S2', 2, 8, 2, 2, 2, 3, PRECISES, build_small(2, 8, 2, 45), claim_clipped),
    ModesCase('seams-S64', 64, SEAM_D, SEAM_J, 1, 8, 0, PRECISES, build_seams(64), claim_seams),
    ModesCase('seams-S72', 72, SEAM_D, SEAM_J, 1, 8, 0, (2,), build_seams(72), claim_seams),
    ModesCase('seams-S80', 80, SEAM_D, SEAM_J, 1, 8, 0, (0, 1), build_seams(80), claim_seams),
    ModesCase('seams-S84', 84, SEAM_D, SEAM_J, 1, 8, 0, (0, 1), build_seams(84), claim_seams),
    ModesCase('tail-S3-D1', 3, 1, 3, 2, 2, 0, PRECISES, build_tail(3, 1), claim_tail),
    ModesCase('tail-S3-D3', 3, 3, 3, 2, 2, 0, PRECISES, build_tail(3, 3), claim_tail),
]
MODES_BY_NAME = {c.name: c for c in MODES_CASES}


@functools.lru_cache(maxsize=None)
def modes_case_logits(name, logit_bytes):
    lg = MODES_BY_NAME[name].build(logit_bytes)
    lg.setflags(write=False)
    return lg


@functools.lru_cache(maxsize=None)
def modes_case_reference(name, logit_bytes):
    c = MODES_BY_NAME[name]
    voxel, stats = MR.modes(modes_case_logits(name, logit_bytes), c.j, c.d, c.perm, c.k, c.radius)
    voxel.setflags(write=False)
    stats.setflags(write=False)
    return voxel, stats


def logit_bytes_of(precise):
    return 8 if precise == 2 else 4


# one bad voxel: (crop, head joint) (1, 1) of a 12 x 12 x 8 volume, in the first voxel, the last, and one of thread 255
BAD_SIDE, BAD_D, BAD_J, BAD_K, BAD_R = 12, 8, 3, 3, 1
BAD_VOXELS = (0, BAD_SIDE * BAD_SIDE * BAD_D - 1, 1022)


class PosteriorCase(NamedTuple):
    name: str
    side: int
    d: int
    j: int
    n: int
    precises: Tuple[int, ...]
    build: Callable            # () -> (logits fp64 [n, S, S, D*J] of fp32 values, prior fp32 [n, Jout, 9])
    claim: Callable            # (case, logits, prior, ref)

    @property
    def perm(self):
        return repeat_last(self.j)


def four_kinds(n, j):
    """Prior rows [n, j + 1, 9] for the permutation repeat_last(j): the four kinds of tests/test_gpu_heat_posterior.py's make_prior
    over (crop + row), the last row that of its twin (the same head joint under the same prior: the same bits)."""
    from tests.test_gpu_heat_posterior import make_prior
    prior = make_prior(n, j + 1, torch.device('cpu')).numpy().copy()
    prior[:, j] = prior[:, j - 1]
    return prior


def kinds_of(n, j):
    from tests.test_gpu_heat_posterior import row_kinds
    kind = row_kinds(n, j + 1).copy()
    kind[:, j] = kind[:, j - 1]
    return kind


def build_post_shape(side, d, j, n):
    def build():
        rng = np.random.default_rng([61, side, d, j])
        lg = fp32_values(rng.standard_normal((n, side, side, d * j)) * (1.0, 6.0)[side % 2] + rng.uniform(-30, 30))
        return lg, four_kinds(n, j)
    return build


def claim_post_shape(case, lg, prior, ref):
    kind = kinds_of(case.n, case.j)
    assert np.isfinite(ref).all() and (np.abs(ref[kind == 1][:, 0]) < 1e-12).all() and (ref[kind == 3][:, 0] < -700).all()


SHARP, FAR = 1e8, 1e4


def build_extremes(side, d):
    """Head joint 0 under a precision of 1e8 about a grid point, 1 under one of 1e4 about (1.5, 1.5, 1.5) (w about -3750 at the
    nearest corner, -33 750 at the farthest: exp(w) is 0 in every format, exp(w - M') is not), 2 finite in its last voxel only."""
    def build():
        j, n = 3, 2
        rng = np.random.default_rng([67, side, d])
        lg = fp32_values(rng.standard_normal((n, side, side, d * j)) * 3)
        vol5(lg, d, j)[..., 2] = -np.inf
        vol5(lg, d, j)[:, side - 1, side - 1, d - 1, 2] = fp32_values(rng.standard_normal(n))
        gs, gd = PR.lin01(side), PR.lin01(d)
        mu = np.zeros((n, j + 1, 3))
        lam = np.zeros((n, j + 1, 3, 3))
        for i in range(n):
            at = (side // 3 + i, side // 2, d // 2)                                 # (x, y, d) indices of the grid point
            mu[i, 0] = (gs[at[0]], gs[at[1]], gd[at[2]])
            lam[i, 0] = np.eye(3) * SHARP
            mu[i, 1] = 1.5
            lam[i, 1] = np.eye(3) * FAR
        a = rng.standard_normal((n, 2, 3, 3))
        mu[:, 2:] = rng.uniform(0, 1, (n, 2, 3))
        lam[:, 2:] = np.einsum('...ab,...cb->...ac', a, a) * 40.0
        mu[:, 3], lam[:, 3] = mu[:, 2], lam[:, 2]                                   # the twin row: the same prior
        return lg, PR.prior_rows(mu, lam).astype(np.float32)
    return build


def claim_extremes(case, lg, prior, ref):
    gs, gd = PR.lin01(case.side), PR.lin01(case.d)
    assert np.isfinite(ref).all()
    for i in range(case.n):
        assert abs(ref[i, 0, 1] - 1) < 1e-9 and (ref[i, 0, 5:8] >= 0).all() and np.abs(ref[i, 0, 5:]).max() < 1e-12       # that voxel
        assert np.array_equal(ref[i, 0, 2:5], prior[i, 0, :3].astype(np.float64))
        assert -40000 < ref[i, 1, 0] < -3000 and abs(ref[i, 1, 1] - 1) < 1e-9                                               # finite, far
        assert np.allclose(ref[i, 1, 2:5], [gs[-1], gs[-1], gd[-1]], atol=1e-9)
        for r in (2, 3):                                                                                                   # the last voxel
            assert ref[i, r, 1] == 1 and np.array_equal(ref[i, r, 2:5], [gs[-1], gs[-1], gd[-1]]) and (ref[i, r, 5:] == 0).all()


POSTERIOR_CASES = [
    PosteriorCase('S45', 45, 8, 3, 2, (0, 1), build_post_shape(45, 8, 3, 2), claim_post_shape),
    PosteriorCase('S46', 46, 8, 3, 2, (0, 1), build_post_shape(46, 8, 3, 2), claim_post_shape),
    PosteriorCase('S31', 31, 8, 3, 2, (2,), build_post_shape(31, 8, 3, 2), claim_post_shape),
    PosteriorCase('S32', 32, 8, 3, 2, (2,), build_post_shape(32, 8, 3, 2), claim_post_shape),
    PosteriorCase('S1', 1, 8, 3, 2, PRECISES, build_post_shape(1, 8, 3, 2), claim_post_shape),
    PosteriorCase('S128', 128, 8, 17, 1, PRECISES, build_post_shape(128, 8, 17, 1), claim_post_shape),
    PosteriorCase('extremes-S16', 16, 8, 3, 2, PRECISES, build_extremes(16, 8), claim_extremes),
    PosteriorCase('extremes-S46', 46, 8, 3, 2, PRECISES, build_extremes(46, 8), claim_extremes),
]
POSTERIOR_BY_NAME = {c.name: c for c in POSTERIOR_CASES}


@functools.lru_cache(maxsize=None)
def posterior_case(name):
    c = POSTERIOR_BY_NAME[name]
    lg, prior = c.build()
    ref = PR.posterior(lg, c.j, c.d, c.perm, prior)
    for a in (lg, prior, ref):
        a.setflags(write=False)
    return lg, prior, ref


class MarginalsCase(NamedTuple):
    name: str
    side: int
    j: int
    d: int
    n: int
    holes: bool = False        # head joint 0: a channel of -Inf only inside a finite joint; head joint 1: -Inf only

    @property
    def perm(self):
        return repeat_last(self.j)


MARGINALS_CASES = [
    MarginalsCase('S2', 2, 17, 8, 2), MarginalsCase('S45', 45, 17, 8, 1), MarginalsCase('S46', 46, 17, 8, 1),
    MarginalsCase('S46-j53', 46, 53, 8, 1), MarginalsCase('S48-j53', 48, 53, 8, 1), MarginalsCase('S18', 18, 19, 8, 2),
    MarginalsCase('S128', 128, 17, 8, 1), MarginalsCase('S7-j53', 7, 53, 8, 2), MarginalsCase('S16-j53', 16, 53, 8, 1),
    MarginalsCase('S3-j1-d1', 3, 1, 1, 2), MarginalsCase('S9-holes', 9, 3, 4, 2, True), MarginalsCase('S46-holes', 46, 3, 8, 1, True),
]
MARGINALS_BY_NAME = {c.name: c for c in MARGINALS_CASES}


@functools.lru_cache(maxsize=None)
def marginals_case(name):
    """-> (logits of fp32 values, ref xy, ref z)."""
    c = MARGINALS_BY_NAME[name]
    rng = np.random.default_rng([71, c.side, c.j, c.d])
    lg = fp32_values(rng.standard_normal((c.n, c.side, c.side, c.d * c.j)) * (1.0, 8.0)[(c.side + c.j) % 2] + rng.uniform(-30, 30))
    if c.holes:
        vol5(lg, c.d, c.j)[..., 1, 0] = -np.inf
        vol5(lg, c.d, c.j)[..., 1] = -np.inf
    rxy, rz = HR.marginals(lg, c.j, c.d, c.perm)
    for a in (lg, rxy, rz):
        a.setflags(write=False)
    return lg, rxy, rz


@functools.lru_cache(maxsize=None)
def host_marginals_case(side, j, d, n, wide):
    lg = TH.case_logits(side, j, d, n, 2 if wide else 0)
    rxy, rz = HR.marginals(lg, j, d, TH.case_permutation(j))
    for a in (lg, rxy, rz):
        a.setflags(write=False)
    return lg, rxy, rz


def launches():
    """[(kernel, case id, side, joints, depth, precise)]: every (case, precise) this file launches, for the closure."""
    out = []
    for side, j, d, n, k, radius, _ in TM.HOST_CASES:
        out += [('modes', f'host-{side}-{j}-{d}-{n}-{k}-{radius}', side, j, d, p) for p in PRECISES]
    for c in MODES_CASES:
        out += [('modes', c.name, c.side, c.j, c.d, p) for p in c.precises]
    for side, d, j in TP.HOST_SHAPES:
        out += [('posterior', f'host-{side}-{d}-{j}', side, j, d, p) for p in PRECISES]
    for c in POSTERIOR_CASES:
        out += [('posterior', c.name, c.side, c.j, c.d, p) for p in c.precises]
    for side, j, d, n in TH.HOST_CASES:
        out += [('marginals', f'host-{side}-{j}-{d}-{n}', side, j, d, p) for p in PRECISES]
    for c in MARGINALS_CASES:
        out += [('marginals', c.name, c.side, c.j, c.d, p) for p in PRECISES]
    return out


def shape_class(kernel, side, j, d, precise):
    return {'modes': lambda: modes_class(side, d, precise), 'posterior': lambda: posterior_class(side, d, precise),
            'marginals': lambda: marginals_class(side, j, d, precise)}[kernel]()


# ---- running the entries -------------------------------------------------------------------------------------------------------

def make_spec(side, j, d, perm):
    cs = _lib.MetroSpec()
    cs.arch, cs.stride, cs.n_joints_head, cs.depth, cs.centered_stride, cs.proc_side = 50, 32, j, d, 1, 32 * side
    cs.box_size_mm, cs.base_width, cs.precision, cs.n_joints_out = 2200.0, 64, 0, len(perm)
    for i, p in enumerate(perm):
        cs.permutation[i] = p
    return cs


def upload(lg, precise, cuda):
    return torch.from_numpy(np.array(lg, np.float64 if precise == 2 else np.float32, order='C')).to(cuda)       # a writable copy


class Padded:
    """An output of `shape` with PAD sentinel words in front of it and behind it."""

    def __init__(self, shape, dtype, cuda):
        self.count = int(np.prod(shape))
        self.shape = tuple(shape)
        self.all = torch.full((PAD + self.count + PAD,), SENTINEL, dtype=dtype, device=cuda)
        self.ptr = C.c_void_p(self.all.data_ptr() + PAD * 4)

    def take(self, what):
        a = self.all.cpu()
        assert (a[:PAD] == SENTINEL).all() and (a[PAD + self.count:] == SENTINEL).all(), (what, 'a sentinel around the rows was overwritten')
        return a[PAD:PAD + self.count].reshape(self.shape).numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def twin_rows_agree(perm, *outs):
    """Two output rows that name the same head joint carry the same bits."""
    first = {}
    for r, p in enumerate(perm):
        if p in first:
            for o in outs:
                assert same_bits(o[:, r], o[:, first[p]]), ('rows', first[p], r, 'of head joint', p)
        first.setdefault(p, r)


def run_marginals(lib, cuda, lg, j, d, perm, precise):
    n, side = lg.shape[:2]
    cs, t = make_spec(side, j, d, perm), upload(lg, precise, cuda)
    scratch = torch.empty(lib.metro_heat_marginals_scratch_bytes(C.byref(cs), n), dtype=torch.uint8, device=cuda)
    xy, z = Padded((n, len(perm), side, side), torch.float32, cuda), Padded((n, len(perm), d), torch.float32, cuda)
    check(lib.metro_heat_marginals(C.c_void_p(t.data_ptr()), n, C.byref(cs), precise, C.c_void_p(scratch.data_ptr()), xy.ptr, z.ptr, None),
          'metro_heat_marginals')
    torch.cuda.synchronize()
    out = xy.take('xy'), z.take('z')
    twin_rows_agree(perm, *out)
    return out


def run_modes(lib, cuda, lg, j, d, perm, k, radius, precise):
    n, side = lg.shape[:2]
    cs, t = make_spec(side, j, d, perm), upload(lg, precise, cuda)
    voxel, stats = Padded((n, len(perm), k), torch.int32, cuda), Padded((n, len(perm), k, MR.STATS), torch.float32, cuda)
    check(lib.metro_heat_modes(C.c_void_p(t.data_ptr()), n, C.byref(cs), precise, k, radius, voxel.ptr, stats.ptr, None), 'metro_heat_modes')
    torch.cuda.synchronize()
    out = voxel.take('voxel'), stats.take('stats')
    twin_rows_agree(perm, *out)
    return out


def run_posterior(lib, cuda, lg, prior, j, d, perm, precise):
    n, side = lg.shape[:2]
    cs, t = make_spec(side, j, d, perm), upload(lg, precise, cuda)
    pr = torch.from_numpy(np.array(prior, np.float32, order='C')).to(cuda)
    assert tuple(pr.shape) == (n, len(perm), PR.PRIOR)
    post = Padded((n, len(perm), PR.STATS), torch.float32, cuda)
    check(lib.metro_heat_posterior(C.c_void_p(t.data_ptr()), n, C.byref(cs), precise, C.c_void_p(pr.data_ptr()), post.ptr, None),
          'metro_heat_posterior')
    torch.cuda.synchronize()
    out = post.take('post')
    prior = np.ascontiguousarray(prior, np.float32)
    for r, p in enumerate(perm):                        # two rows of one head joint under the same prior row: the same bits
        if perm.index(p) != r and same_bits(prior[:, r], prior[:, perm.index(p)]):
            assert same_bits(out[:, r], out[:, perm.index(p)]), ('rows', perm.index(p), r, 'of head joint', p)
    return out


# ---- the figures ---------------------------------------------------------------------------------------------------------------

def finite_rows(xy, z, rxy, rz):
    """The marginals with the rows that are NaN in the restatement (a joint of -Inf only) set to 1 on both sides, after holding
    the kernel to exactly those rows."""
    off = np.isnan(rz).any(-1)
    assert np.array_equal(np.isnan(xy).any((2, 3)), off) and np.array_equal(np.isnan(z).any(-1), off)
    assert np.array_equal(np.isnan(xy).all((2, 3)), off) and np.array_equal(np.isnan(z).all(-1), off) and np.array_equal(np.isnan(rxy).all((2, 3)), off)
    fill = lambda a: np.where(off.reshape(off.shape + (1,) * (a.ndim - 2)), 1.0, a)
    return fill(xy), fill(z), fill(rxy), fill(rz)


def marginals_runs(lib, cuda, precise, shared):
    """(what, voxels of a joint, xy, z, ref xy, ref z) of every marginals case: the host list (`shared`) or this file's own."""
    if shared:
        for side, j, d, n in TH.HOST_CASES:
            lg, rxy, rz = host_marginals_case(side, j, d, n, precise == 2)
            yield (f'host S{side} J{j} D{d} n{n}', side * side * d) + finite_rows(*run_marginals(lib, cuda, lg, j, d, TH.case_permutation(j), precise), rxy, rz)
    else:
        for c in MARGINALS_CASES:
            lg, rxy, rz = marginals_case(c.name)
            yield (c.name, c.side * c.side * c.d) + finite_rows(*run_marginals(lib, cuda, lg, c.j, c.d, c.perm, precise), rxy, rz)


def modes_runs(lib, cuda, precise, shared):
    """(what, side, depth, voxel, stats, ref voxel, ref stats) of every modes case."""
    if shared:
        for side, j, d, n, k, radius, _ in TM.HOST_CASES:
            lg = TM.case_logits(side, j, d, n, precise == 2)
            rv, rs = TM.case_reference(side, j, d, n, k, radius, precise == 2)
            yield (f'host S{side} J{j} D{d} n{n} K{k} R{radius}', side, d) + run_modes(lib, cuda, lg, j, d, TM.case_permutation(j), k, radius, precise) + (rv, rs)
    else:
        for c in MODES_CASES:
            if precise in c.precises:
                b = logit_bytes_of(precise)
                yield (c.name, c.side, c.d) + run_modes(lib, cuda, modes_case_logits(c.name, b), c.j, c.d, c.perm, c.k, c.radius, precise) + \
                    modes_case_reference(c.name, b)


def posterior_runs(lib, cuda, precise, shared):
    """(what, side, depth, post, ref) of every posterior case."""
    if shared:
        for side, d, j in TP.HOST_SHAPES:
            for scenario in TP.SCENARIOS:
                lg, prior = TP.case(side, d, j, scenario, precise == 2)
                yield (f'host S{side} D{d} J{j} {scenario}', side, d, run_posterior(lib, cuda, lg, prior, j, d, TP.real_permutation(j), precise),
                       TP.case_reference(side, d, j, scenario, precise == 2))
    else:
        for c in POSTERIOR_CASES:
            if precise in c.precises:
                lg, prior, ref = posterior_case(c.name)
                yield c.name, c.side, c.d, run_posterior(lib, cuda, lg, prior, c.j, c.d, c.perm, precise), ref


def worst_of(figures):
    out = {}
    for f in figures:
        out = {m: max(out.get(m, 0.0), f[m]) for m in f}
    return out


def kernel_deviations(lib, cuda, kernel, precise, shared):
    """The worst figures of one kernel over one of the two lists (marginals: {'abs', 'rel', 'voxels'})."""
    if kernel == 'marginals':
        figs, voxels = [], []
        for what, vox, xy, z, rxy, rz in marginals_runs(lib, cuda, precise, shared):
            for got, ref in ((xy, rxy), (z, rz)):
                a, r = HR.deviation(got, ref)
                figs.append({'abs': a, 'rel': r})
            voxels.append(vox)
        return dict(worst_of(figs), voxels=min(voxels))
    if kernel == 'modes':
        figs = []
        for what, side, d, voxel, stats, rv, rs in modes_runs(lib, cuda, precise, shared):
            assert np.array_equal(voxel, rv), (what, 'voxel')
            figs.append(MR.deviation(stats, rv, rs, side, d))
        return worst_of(figs)
    return worst_of(PR.deviation(post, ref, side, d) for what, side, d, post, ref in posterior_runs(lib, cuda, precise, shared))


def gpu_deviations(cuda, kernel):
    """{key: figures} of every comparison of this file for one kernel ('marginals': (abs, rel, smallest voxels), as
    tests/test_gpu_heat_marginals.py gives them): what tools/heat_*_parity.py record under the gpu/acc* keys."""
    lib = _lib.load()
    out = {}
    for precise in PRECISES:
        parts = [kernel_deviations(lib, cuda, kernel, precise, shared) for shared in (True, False)]
        for shared, p in zip(('host lists', 'own cases'), parts):
            print(f'heat_{kernel} {KEYS[precise]} {shared}: ' + ' '.join(f'{m} {p[m]:.3e}' for m in p), flush=True)
        if kernel == 'marginals':
            out[KEYS[precise]] = (max(p['abs'] for p in parts), max(p['rel'] for p in parts), min(p['voxels'] for p in parts))
        else:
            out[KEYS[precise]] = worst_of(parts)
    return out


def rounding_deviation(refs):
    """The posterior figures of the restatement's own rounding to fp32: what an exact fp64 sum stored as fp32 deviates by."""
    return worst_of(PR.deviation(ref.astype(np.float32), ref, side, d) for side, d, ref in refs)


# ---- a: the host lists on the device -------------------------------------------------------------------------------------------

def hold_modes(what, side, d, voxel, stats, rv, rs, key):
    small = MR.small_fraction(rv, rs)
    assert small < 0.05, (what, small)
    MR.check(voxel, stats, rv, rs, side, d, key, what)
    assert (np.nansum(stats[..., 0].astype(np.float64), -1) <= 1 + 1e-5).all(), what


@pytest.mark.parametrize('precise', PRECISES)
def test_modes_host_cases_on_the_device(cuda, lib, precise):
    figs = []
    for what, side, d, voxel, stats, rv, rs in modes_runs(lib, cuda, precise, True):
        hold_modes(what, side, d, voxel, stats, rv, rs, KEYS[precise])
        figs.append(MR.deviation(stats, rv, rs, side, d))
    if precise in HOST_KEYS:
        worst, host = worst_of(figs), MR.recorded()['worst'][HOST_KEYS[precise]]
        print(f'heat_modes {KEYS[precise]} on the host list: {worst}; the host walk recorded {host}')
        assert all(worst[m] <= 2 * host[m] for m in worst), (worst, host)


@pytest.mark.parametrize('precise', PRECISES)
def test_posterior_host_cases_on_the_device(cuda, lib, precise):
    figs, refs = [], []
    for what, side, d, post, ref in posterior_runs(lib, cuda, precise, True):
        PR.check(post, ref, side, d, PR.gate(KEYS[precise]), KEYS[precise], what)
        nan_rows = np.isnan(post).any(-1)
        assert np.array_equal(nan_rows, np.isnan(post).all(-1)) and np.array_equal(nan_rows, np.isnan(ref).any(-1)), what
        if what.endswith(' zero'):
            assert (post[0, :, 0] == 0.0).all() and not np.signbit(post[0, :, 0]).any(), what
        if what.endswith(' far'):
            assert np.isfinite(post).all() and (post[..., 0] < -700).all() and (post[..., 0] > -2000).all(), what
        figs.append(PR.deviation(post, ref, side, d))
        refs.append((side, d, ref))
    if precise in HOST_KEYS:
        worst, rounding = worst_of(figs), rounding_deviation(refs)
        print(f'heat_posterior {KEYS[precise]} on the host list: {worst}; the restatement rounded to fp32: {rounding}')
        assert all(worst[m] <= 2 * rounding[m] for m in worst), (worst, rounding)


@pytest.mark.parametrize('precise', PRECISES)
def test_marginals_host_cases_on_the_device(cuda, lib, precise):
    rec = HR.recorded()
    worst = [0.0, 0.0]
    for what, vox, xy, z, rxy, rz in marginals_runs(lib, cuda, precise, True):
        HR.check(xy, z, rxy, rz, KEYS[precise], rec['smallest_voxels'][KEYS[precise]], what)
        assert np.allclose(xy.astype(np.float64).sum((2, 3)), 1, atol=1e-5) and np.allclose(z.astype(np.float64).sum(2), 1, atol=1e-5), what
        for got, ref in ((xy, rxy), (z, rz)):
            worst = [max(w, f) for w, f in zip(worst, HR.deviation(got, ref))]
    if precise in HOST_KEYS:
        host = rec['worst'][HOST_KEYS[precise]]
        print(f'heat_marginals {KEYS[precise]} on the host list: abs {worst[0]:.3e} rel {worst[1]:.3e}; the host walk recorded {host}')
        assert worst[0] <= 2 * host['abs'] and worst[1] <= 2 * host['rel'], (worst, host)


# ---- b: the workgroup cases of the modes ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,precise', [(c.name, p) for c in MODES_CASES for p in c.precises])
def test_modes_workgroup_cases(cuda, lib, name, precise):
    c = MODES_BY_NAME[name]
    b = logit_bytes_of(precise)
    lg, (rv, rs) = modes_case_logits(name, b), modes_case_reference(name, b)
    c.claim(c, lg, rv, rs, b)
    voxel, stats = run_modes(lib, cuda, lg, c.j, c.d, c.perm, c.k, c.radius, precise)
    hold_modes(name, c.side, c.d, voxel, stats, rv, rs, KEYS[precise])


@pytest.mark.parametrize('precise', PRECISES)
def test_modes_one_bad_voxel_poisons_its_joint_only(cuda, lib, precise):
    rng = np.random.default_rng(59)
    clean = fp32_values(rng.standard_normal((2, BAD_SIDE, BAD_SIDE, BAD_D * BAD_J)) * 2)
    perm = repeat_last(BAD_J)
    cv, cs = run_modes(lib, cuda, clean, BAD_J, BAD_D, perm, BAD_K, BAD_R, precise)
    rv, rs = MR.modes(clean, BAD_J, BAD_D, perm, BAD_K, BAD_R)
    hold_modes('clean', BAD_SIDE, BAD_D, cv, cs, rv, rs, KEYS[precise])
    assert owner(BAD_VOXELS[2]) == (255, 3, 63)
    keep = np.ones((2, len(perm)), bool)
    keep[1, 1] = False
    for bad in (np.nan, np.inf):
        for v in BAD_VOXELS:
            lg = clean.copy()
            vol5(lg, BAD_D, BAD_J)[(1,) + lin(v, BAD_SIDE, BAD_D) + (1,)] = bad
            voxel, stats = run_modes(lib, cuda, lg, BAD_J, BAD_D, perm, BAD_K, BAD_R, precise)
            assert (voxel[1, 1] == -1).all() and np.isnan(stats[1, 1]).all(), (bad, v)
            assert same_bits(voxel[keep], cv[keep]) and same_bits(stats[keep], cs[keep]), (bad, v)


# ---- c: the posterior's shapes and extremes ------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,precise', [(c.name, p) for c in POSTERIOR_CASES for p in c.precises])
def test_posterior_shapes_and_extremes(cuda, lib, name, precise):
    c = POSTERIOR_BY_NAME[name]
    lg, prior, ref = posterior_case(name)
    c.claim(c, lg, prior, ref)
    assert same_bits(prior[:, c.j], prior[:, c.j - 1])                      # run_posterior holds the twin rows to the same bits
    post = run_posterior(lib, cuda, lg, prior, c.j, c.d, c.perm, precise)
    PR.check(post, ref, c.side, c.d, PR.gate(KEYS[precise]), KEYS[precise], name)
    if c.claim is claim_post_shape:
        kind = kinds_of(c.n, c.j)
        assert (post[kind == 1][:, 0] == 0.0).all(), 'a zero precision: log_evidence exactly 0'
        assert (post[kind == 3][:, 0] < -700).all(), 'a prior far outside the volume'
    else:
        assert (post[:, 0, 5:8] >= 0).all() and (post[:, 0, 1] > 0.999).all(), 'the sharp prior: one voxel, no negative variance'


# ---- d: the marginals' shapes --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('precise', PRECISES)
@pytest.mark.parametrize('name', [c.name for c in MARGINALS_CASES])
def test_marginals_shapes(cuda, lib, name, precise):
    c = MARGINALS_BY_NAME[name]
    lg, rxy, rz = marginals_case(name)
    xy, z = run_marginals(lib, cuda, lg, c.j, c.d, c.perm, precise)
    off = np.isnan(rz).any(-1)
    assert off.any() == c.holes and (not c.holes or np.array_equal(off, np.broadcast_to(np.array(c.perm) == 1, off.shape)))
    fxy, fz, frxy, frz = finite_rows(xy, z, rxy, rz)
    HR.check(fxy, fz, frxy, frz, KEYS[precise], HR.recorded()['smallest_voxels'][KEYS[precise]], name)
    sums_xy, sums_z = xy.astype(np.float64).sum((2, 3))[~off], z.astype(np.float64).sum(2)[~off]
    assert np.allclose(sums_xy, 1, atol=1e-5) and np.allclose(sums_z, 1, atol=1e-5), (name, np.abs(sums_xy - 1).max(), np.abs(sums_z - 1).max())
    if c.holes:
        assert (z[:, 0, 1] == 0).all() and np.isfinite(z[:, 0]).all()                 # the channel of -Inf only: weight zero


# ---- e: bits -------------------------------------------------------------------------------------------------------------------

BITS_SHAPES = ((16, 3, 8), (46, 2, 8))        # staged whole / tile 32, and streamed / slabs / tile 64


@pytest.mark.parametrize('precise', PRECISES)
@pytest.mark.parametrize('side,j,d', BITS_SHAPES)
def test_a_crops_position_in_the_call_does_not_change_its_bits(cuda, lib, side, j, d, precise):
    rng = np.random.default_rng([73, side])
    crops = fp32_values(rng.standard_normal((5, side, side, d * j)) * 3)
    perm, k, radius = repeat_last(j), 4, 1
    prior = four_kinds(5, j)
    calls = {'alone': [0], 'first of 3': [0, 1, 2], 'last of 3': [3, 4, 0]}
    got = {}
    for what, rows in calls.items():
        at = rows.index(0)
        pr = prior[rows]
        xy, z = run_marginals(lib, cuda, crops[rows], j, d, perm, precise)
        voxel, stats = run_modes(lib, cuda, crops[rows], j, d, perm, k, radius, precise)
        post = run_posterior(lib, cuda, crops[rows], pr, j, d, perm, precise)
        got[what] = [a[at] for a in (xy, z, voxel, stats, post)]
    for what in ('first of 3', 'last of 3'):
        for name, a, b in zip(('xy', 'z', 'voxel', 'stats', 'post'), got['alone'], got[what]):
            assert same_bits(a, b), (what, name)


@pytest.mark.parametrize('precision,precise', (('f16', 0), ('f64', 2)))
@pytest.mark.parametrize('head', ('S16-j17', 'S64'))
def test_the_bound_forward_gives_the_bits_of_the_entries_on_its_own_logits(cuda, lib, head, precision, precise):
    """What carries the crafted results over to metro_forward: the sums have a fixed order and no atomics, so the bound forward's
    marginals, modes and posterior are, bit for bit, what the entries give on the dumped logits of that forward."""
    from metro_pose3d_amd import synth
    from metro_pose3d_amd.engine import Engine
    from tests import test_gpu_heat_posterior as GP
    spec, params, ns = GP.make_case(head)
    n, (k, radius) = ns[-1], GP.MODES_KR
    eng = Engine(spec, params, precision, max_batch=n, device=cuda)
    x = torch.from_numpy(synth.make_images(n, spec.proc_side, seed=7)).to(cuda)
    prior = GP.make_prior(n, spec.skeleton.n_out, cuda)
    heat = GP.buffers(eng, n, cuda, heat=True)
    eng.forward(x, **heat)
    _, voxel, stats = eng.forward_modes(x, k, radius)
    _, post = eng.forward_posterior(x, prior)
    dump = eng.forward_upto(x, len(eng.layer_infos()) - 2)
    assert dump.dtype == (torch.float64 if precise == 2 else torch.float32)
    lg = dump.cpu().numpy().astype(np.float64)
    j, d, perm = spec.skeleton.n_head, spec.depth, list(spec.skeleton.permutation)
    xy, z = run_marginals(lib, cuda, lg, j, d, perm, precise)
    ev, es = run_modes(lib, cuda, lg, j, d, perm, k, radius, precise)
    ep = run_posterior(lib, cuda, lg, prior.cpu().numpy(), j, d, perm, precise)
    assert same_bits(heat['heat_xy'].cpu().numpy(), xy) and same_bits(heat['heat_z'].cpu().numpy(), z)
    assert same_bits(voxel.cpu().numpy(), ev) and same_bits(stats.cpu().numpy(), es)
    assert same_bits(post.cpu().numpy(), ep)
    eng.close()
