"""The batch layout of the real-batch parity tests (tests/helpers.py: crop_assignment, lay_out_twins, assert_twins) -- CPU only.

test_kernel_coverage.py and the {'batch': N} cases of test_f16_layerwise.py build a call of n crops from p images, hold the first
p positions to an oracle and every other position to the bits of its twin.  That carries the oracle to the whole call only if no
misplacement of results maps the layout onto itself; here the layout's properties are checked for every (n, p) those tests use,
and whole-tile faults are planted into a synthetic output to see the twin check fail."""
import zlib

import numpy as np
import pytest
import torch

from tests import helpers as H

# (n, p): test_kernel_coverage.py's batches at p = min(4, n), and the real-batch cases of test_f16_layerwise.py (two oracle crops)
# (+ odd call sizes of the single launches and the ragged real-batch cases)
COVERAGE_BATCHES = (1, 8, 16, 32, 64, 130, 256, 13, 31, 49, 63, 101, 135, 253)
PAIRS = [(n, min(4, n)) for n in COVERAGE_BATCHES] + [(16, 2), (32, 2), (64, 2), (130, 2), (256, 2), (5, 2), (13, 2), (63, 2)]
SEEDS = (0, 1, zlib.crc32(b'C4-rn101-s8-J19-b32/block3/unit_2/conv2'))
ROTATIONS = (1, 2, 4, 8, 16)


def _output(assign, p, seed=0):
    """A launch that does what it should: out[i] = table[assign[i]], fp32 with a NaN in every row (ReLU-free garbage is legal)."""
    table = torch.from_numpy(np.random.default_rng(seed).standard_normal((p, 5)).astype(np.float32))
    table[:, 2] = float('nan')
    return table[torch.as_tensor(assign)]


def _swap_groups(out, g, k):
    """Groups k and k + 1 of g images exchanged: two blocks swap tiles / tile t lands in tile t + 1's slot and back."""
    out = out.clone()
    out[k * g:(k + 1) * g], out[(k + 1) * g:(k + 2) * g] = out[(k + 1) * g:(k + 2) * g].clone(), out[k * g:(k + 1) * g].clone()
    return out


def _caught(out, assign, p):
    try:
        H.assert_twins(out, assign, p, 'planted')
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize('seed', SEEDS)
@pytest.mark.parametrize('n,p', PAIRS)
def test_assignment_properties(n, p, seed):
    a = H.crop_assignment(n, p, seed)
    assert a.shape == (n,) and a.dtype.kind == 'i'
    assert np.array_equal(a, H.crop_assignment(n, p, seed)), 'not deterministic'
    assert np.array_equal(a[:p], np.arange(p))
    if n <= p:
        return
    assert a[n - 1] == p - 1 and a[0] != a[n - 1]
    assert set(a.tolist()) == set(range(p))
    for s in range(1, n):
        assert (a[:n - s] != a[s:]).any(), f'shift {s}'
    for g in H.TWIN_GROUPS:
        if 2 * g <= n:
            groups = a[:n // g * g].reshape(-1, g)
            assert ((groups[:-1] != groups[1:]).any(axis=1)).all(), f'groups of {g}'


def test_assignment_is_the_identity_up_to_p_images_and_needs_two_base_images_beyond():
    assert np.array_equal(H.crop_assignment(1, 4, 7), [0]) and np.array_equal(H.crop_assignment(4, 4, 7), [0, 1, 2, 3])
    with pytest.raises(ValueError):
        H.crop_assignment(8, 1, 0)


def test_lay_out_twins_on_both_kinds_of_base():
    a = H.crop_assignment(8, 4, 3)
    base = np.arange(4 * 6, dtype=np.float32).reshape(4, 2, 3)
    assert np.array_equal(H.lay_out_twins(base, a), base[a])
    got = H.lay_out_twins(torch.from_numpy(base), a)
    assert got.is_contiguous() and np.array_equal(got.numpy(), base[a])


@pytest.mark.parametrize('n,p', [c for c in PAIRS if c[0] > c[1]])
def test_twin_check_passes_a_right_output_and_catches_rotations(n, p):
    for seed in SEEDS:
        a = H.crop_assignment(n, p, seed)
        for dtype in (torch.float32, torch.float16, torch.int32):
            out = _output(a, p, seed).nan_to_num(7.0).to(dtype) if dtype is torch.int32 else _output(a, p, seed).to(dtype)
            H.assert_twins(out, a, p, 'as it should be')
        out = _output(a, p, seed)
        for g in ROTATIONS:
            if g < n:
                for shift in (g, -g):
                    assert _caught(torch.roll(out, shift, 0), a, p), f'seed {seed}: a rotation of the batch by {shift} images passes'


@pytest.mark.parametrize('n,p', [c for c in PAIRS if c[0] > c[1]])
def test_twin_check_misses_no_swap_of_adjacent_groups(n, p):
    """The cap: the share of planted single-group swaps the check misses is 0 for every group size >= 2 (swaps of two equal
    neighbouring images, g = 1, change nothing and cannot be seen: counted, not asserted)."""
    for seed in SEEDS:
        a = H.crop_assignment(n, p, seed)
        out = _output(a, p, seed)
        for g in H.TWIN_GROUPS:
            missed = [k for k in range(n // g - 1) if not _caught(_swap_groups(out, g, k), a, p)]
            assert not missed, f'seed {seed}: swaps of the {g}-image groups at {[k * g for k in missed]} pass ({len(missed)} of {n // g - 1})'
        equal_neighbours = int((a[:-1] == a[1:]).sum())
        assert [_caught(_swap_groups(out, 1, k), a, p) for k in range(n - 1)].count(False) == equal_neighbours


def test_twin_check_names_the_first_position_that_differs():
    a = H.crop_assignment(32, 4, 0)
    out = _output(a, 4)
    k = next(i for i in range(4, 31) if a[i] != a[i + 1])
    out[[k, k + 1]] = out[[k + 1, k]]
    with pytest.raises(AssertionError, match=f'layer x: position {k} of 32 differs from its twin, position {a[k]}'):
        H.assert_twins(out, a, 4, 'layer x')


@pytest.mark.parametrize('n', [8, 16, 32, 64, 256])
def test_the_periodic_layout_passes_what_the_assignment_catches(n):
    """The hole this layout closes: with image i = image i % 4 a launch that stores every result four images (one 256-pixel tile
    of an 8 x 8 map) further on writes every slot and gives every position its twin's bits."""
    periodic = np.arange(n) % 4
    out = _output(periodic, 4)
    for shift in (4, -4, 8):
        moved = torch.roll(out, shift, 0)
        H.assert_twins(moved, periodic, 4, 'periodic')                                 # blind ...
        assert torch.equal(moved[:4].nan_to_num(0.0), out[:4].nan_to_num(0.0))          # ... and the oracle-checked images are right too
    assert not _caught(_swap_groups(out, 4, 0), periodic, 4)
    a = H.crop_assignment(n, 4, 0)
    out = _output(a, 4)
    assert _caught(torch.roll(out, 4, 0), a, 4) and _caught(torch.roll(out, -4, 0), a, 4) and _caught(_swap_groups(out, 4, 0), a, 4)


@pytest.mark.parametrize('chunk', [1, 5, 12, 35, 64])
def test_the_chunked_twin_check_is_the_whole_one(chunk):
    """Tensors beyond 2^31 elements are gathered and compared in groups of whole images (helpers.TWIN_CHUNK_ELEMENTS): with the
    chunk forced down to a few elements (5 per image here) the layout is the same tensor, a right output passes, and every planted
    swap or rotation is caught with the message of the one-piece check -- the first position that differs."""
    n, p = 49, 4
    a = H.crop_assignment(n, p, 5)
    base = torch.from_numpy(np.random.default_rng(1).standard_normal((p, 5)).astype(np.float32))
    assert torch.equal(H.lay_out_twins(base, a, chunk=chunk), H.lay_out_twins(base, a)) and H.lay_out_twins(base, a, chunk=chunk).is_contiguous()
    out = _output(a, p)
    H.assert_twins(out, a, p, 'as it should be', chunk=chunk)
    planted = [torch.roll(out, s, 0) for s in (1, -1, 4, 16)] + [_swap_groups(out, g, k) for g in H.TWIN_GROUPS for k in (0, n // g - 2)]
    last = out.clone()
    last[n - 1, 4] += 1.0                  # one element of the last image
    for bad in planted + [last]:
        with pytest.raises(AssertionError) as whole:
            H.assert_twins(bad, a, p, 'layer x')
        with pytest.raises(AssertionError) as parts:
            H.assert_twins(bad, a, p, 'layer x', chunk=chunk)
        assert str(parts.value) == str(whole.value)


@pytest.mark.parametrize('n,p,wraps', [(68, 4, [(64, 64), (32, 32)]), (132, 2, [(128, 128)]), (256, 4, [(128, 128), (255, 255)]), (207, 4, [(203, 1)])])
def test_wrap_assignment_puts_different_images_a_wrap_apart(n, p, wraps):
    a, seed = H.wrap_assignment(n, p, 11, wraps)
    assert np.array_equal(a, H.crop_assignment(n, p, seed)) and seed >= 11
    for first, d in wraps:
        assert any(a[i] != a[i - d] for i in range(first, n))
    # a store that wraps at the boundary: the images beyond `first` land `d` lower and their own slots keep the NaN prefill
    first, d = wraps[0]
    out = _output(a, p).nan_to_num(3.0)
    wrapped = out.clone()
    wrapped[first - d:n - d] = out[first:]
    wrapped[first:] = float('nan')
    assert _caught(wrapped, a, p)
    # a load that wraps: the images beyond `first` are computed from the images `d` lower
    wrapped = out.clone()
    wrapped[first:] = out[first - d:n - d]
    assert _caught(wrapped, a, p)
