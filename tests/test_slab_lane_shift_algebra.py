"""The identity behind conv3x3_f16_slab's lane-shift form (slab_tile: HS), on the CPU.  In the kernel's pixel fragment lane l holds tile
pixel l & 31 and k half l >> 5; tiles start at multiples of 256 pixels and fragments at multiples of 32, so on a 16-wide map every 16-lane
DPP row of a fragment is one image row.  Then the side taps (dr, -d) and (dr, +d) of a kernel row are the centre tap (dr, 0)'s fragment
shifted by d lanes inside each 16-lane row with zero fill (row_shr:d / row_shl:d, bound_ctrl) -- TF SAME padding included: the zero the
shift brings in at x < d or x >= 16 - d is the padding.  On 8- and 32-wide maps the identity fails (a DPP row holds two image rows, or half
of one), which is why the launcher takes the form only where the map, or the sub-image in sub-grid order, is 16 wide."""
import numpy as np
import pytest

LANES, FRAG, ROW = 64, 32, 16


def row_shift(v, d):
    """v_mov_b32_dpp row_shr:d (d > 0) / row_shl:-d (d < 0) with bound_ctrl: lane l takes lane l - d of its own 16-lane row, 0 outside it."""
    out = np.zeros_like(v)
    for l in range(LANES):
        src = l % ROW - d
        if 0 <= src < ROW:
            out[l] = v[l - d]
    return out


def tap_fragment(img, frag, dr, ds):
    """The pixel fragment of tap (dr, ds) as the plain form reads it: img [h, w, 2] (the two k halves), fragment `frag` of the image's
    pixels in row-major order; a tap outside the image reads zero."""
    h, w, _ = img.shape
    out = np.zeros(LANES, img.dtype)
    for l in range(LANES):
        p = frag * FRAG + (l & 31)
        y, x = divmod(p, w)
        if 0 <= y + dr < h and 0 <= x + ds < w:
            out[l] = img[y + dr, x + ds, l >> 5]
    return out


def image(h, w):
    # every (pixel, k half) holds its own non-zero value
    return 1 + np.arange(h * w * 2).reshape(h, w, 2)


def side_taps_match(h, w, d, frag, dr):
    img = image(h, w)
    centre = tap_fragment(img, frag, dr, 0)
    return (np.array_equal(row_shift(centre, d), tap_fragment(img, frag, dr, -d)),
            np.array_equal(row_shift(centre, -d), tap_fragment(img, frag, dr, d)))


@pytest.mark.parametrize('d', [1, 2])
@pytest.mark.parametrize('h', [16, 8, 4])
def test_row_shift_of_the_centre_tap_is_the_side_tap_on_16_wide_maps(h, d):
    w = 16
    frags = h * w // FRAG
    for frag in range(frags):                    # the first and last fragments hold the rows at the top and bottom image edge
        for dr in (-d, 0, d):
            left, right = side_taps_match(h, w, d, frag, dr)
            assert left and right, (h, d, frag, dr)
    # both k halves and the edge columns really are in what was compared
    img = image(h, w)
    c = tap_fragment(img, 0, 0, 0)
    assert np.array_equal(c[:32], img.reshape(-1, 2)[:32, 0]) and np.array_equal(c[32:], img.reshape(-1, 2)[:32, 1])
    s = row_shift(c, d)
    assert (s.reshape(4, ROW)[:, :d] == 0).all() and (s.reshape(4, ROW)[:, d:] != 0).all()
    s = row_shift(c, -d)
    assert (s.reshape(4, ROW)[:, ROW - d:] == 0).all() and (s.reshape(4, ROW)[:, :ROW - d] != 0).all()


@pytest.mark.parametrize('d', [1, 2])
@pytest.mark.parametrize('w', [8, 32])
def test_the_identity_fails_on_8_and_32_wide_maps(w, d):
    h = 16
    # interior fragments: every lane's row tap is inside the image
    inner = [f for f in range(h * w // FRAG) if f * FRAG // w >= 2 and (f * FRAG + FRAG - 1) // w <= h - 3]
    for dr in (-d, 0, d):
        for frag in (inner[0], inner[-1]):
            left, right = side_taps_match(h, w, d, frag, dr)
            assert not left and not right, (w, d, frag, dr)
    # width 8: lane 8 is x = 0 of the next image row and takes its neighbour's pixel instead of the padding
    img = image(h, 8)
    c = tap_fragment(img, 1, 0, 0)
    assert row_shift(c, d)[8] == c[8 - d] != 0 and tap_fragment(img, 1, 0, -d)[8] == 0
    # width 32: lane 16 is x = 16 and takes a zero instead of x = 16 - d
    img = image(h, 32)
    c = tap_fragment(img, 1, 0, 0)
    assert row_shift(c, d)[16] == 0 and tap_fragment(img, 1, 0, -d)[16] == c[16 - d] != 0
