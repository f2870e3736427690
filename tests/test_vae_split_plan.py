"""The planner of the exact spatial split of the VAE decode (svi_vae_split_plan; host arithmetic, no GPU).

A part owns a rectangle of the latent grid and decodes, behind the whole-frame middle block, a crop that is its rectangle plus a halo.
The halo entering a stage is what the layers behind that point can still reach.  With random weights a pixel 13 away moves the output
far below fp32 resolution (each step outward keeps about a third of the energy, through ~25 convolutions), so no numerical test can see a
halo one pixel short: the halo is pinned here, structurally, against a restatement of the decoder's layer counts."""
import ctypes as C

import pytest

from svi_hip import _lib as L

GRIDS = [(60, 104), (90, 160), (7, 9), (32, 40)]
SPLITS = [(1, 2), (2, 1), (2, 2), (2, 4), (3, 1)]


def expected_halos():
    """Backwards from the output: the three-tap head convolution needs 1 px; each stage's three residual blocks hold two three-tap
    convolutions each (1 px per convolution: 6); the three-tap resample convolution behind stages 0-2 needs 1 more, and it reads through a
    nearest x2 upsample, which halves the requirement, rounded up.  time_conv and the shortcuts are 1 x 1 in space."""
    res_blocks, convs_per_block, reach = 3, 2, 3 // 2
    need, halos = reach, [0] * 4                       # head
    for stage in (3, 2, 1, 0):
        if stage != 3:                                 # the upsample block between this stage and the next
            need = -(-(need + reach) // 2)
        need += res_blocks * convs_per_block * reach
        halos[stage] = need
    return tuple(halos)


def plans(grid, split):
    return [L.vae_split_plan(*grid, *split, p) for p in range(split[0] * split[1])]


def test_halos_follow_from_the_layer_counts():
    assert expected_halos() == (13, 12, 10, 7)
    for grid in GRIDS:
        for split in SPLITS:
            for pl in plans(grid, split):
                assert pl["halo"] == expected_halos(), (grid, split, pl)


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("split", SPLITS)
def test_owned_rectangles_tile_the_frame(grid, split):
    hh, ww = grid
    ph, pw = split
    cover = [[0] * ww for _ in range(hh)]
    for p, pl in enumerate(plans(grid, split)):
        h0, h1, w0, w1 = pl["owned"]
        i, j = divmod(p, pw)
        assert (h0, h1, w0, w1) == (i * hh // ph, (i + 1) * hh // ph, j * ww // pw, (j + 1) * ww // pw)
        assert h1 > h0 and w1 > w0
        for y in range(h0, h1):
            for x in range(w0, w1):
                cover[y][x] += 1
    assert all(v == 1 for row in cover for v in row)             # disjoint, and nothing left out


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("split", SPLITS)
def test_padded_rectangles_hold_the_halo_and_stop_at_the_border(grid, split):
    hh, ww = grid
    ph, pw = split
    halos = expected_halos()
    for pl in plans(grid, split):
        h0, h1, w0, w1 = pl["owned"]
        for s, (a0, a1, b0, b1) in enumerate(pl["padded"]):
            f, n = 1 << s, halos[s]
            H, W = hh * f, ww * f
            assert 0 <= a0 <= h0 * f and h1 * f <= a1 <= H and 0 <= b0 <= w0 * f and w1 * f <= b1 <= W     # contains the owned rectangle, inside the image
            # an interior cut carries exactly the halo, unless the image border comes first; a side on the border has nothing to add
            assert a0 == (max(h0 * f - n, 0) if h0 > 0 else 0)
            assert a1 == (min(h1 * f + n, H) if h1 < hh else H)
            assert b0 == (max(w0 * f - n, 0) if w0 > 0 else 0)
            assert b1 == (min(w1 * f + n, W) if w1 < ww else W)
        for s in range(1, 4):                                    # each crop is cut from the previous stage's upsampled crop
            q, r = pl["padded"][s - 1], pl["padded"][s]
            assert 2 * q[0] <= r[0] and r[1] <= 2 * q[1] and 2 * q[2] <= r[2] and r[3] <= 2 * q[3]


def test_full_halo_is_exercised_away_from_the_border():
    """At (60, 104) in 2 x 2 both cuts are farther than 13 latent pixels from every border: every interior side extends by exactly the halo."""
    for pl in plans((60, 104), (2, 2)):
        h0, h1, w0, w1 = pl["owned"]
        for s, (a0, a1, b0, b1) in enumerate(pl["padded"]):
            f, n = 1 << s, expected_halos()[s]
            assert (h0 * f - a0, a1 - h1 * f) == ((n, 0) if h0 else (0, n))
            assert (w0 * f - b0, b1 - w1 * f) == ((n, 0) if w0 else (0, n))


@pytest.mark.parametrize("grid", GRIDS)
def test_one_part_is_the_whole_frame_without_halo(grid):
    hh, ww = grid
    pl = L.vae_split_plan(hh, ww, 1, 1, 0)
    assert pl["owned"] == (0, hh, 0, ww) and pl["halo"] == (0, 0, 0, 0)
    assert pl["padded"] == [(0, hh << s, 0, ww << s) for s in range(4)]


@pytest.mark.parametrize("args,word", [((7, 9, 2, 2, 4), "outside"), ((7, 9, 2, 2, -1), "outside"), ((7, 9, 8, 1, 0), "without a pixel"),
                                       ((7, 9, 1, 10, 0), "without a pixel"), ((7, 9, 0, 1, 0), "positive"), ((0, 9, 1, 1, 0), "positive")])
def test_bad_arguments_are_refused_with_a_message(args, word):
    out = (C.c_int32 * 24)()
    assert L.lib().svi_vae_split_plan(*args, out) != 0
    assert word in L.last_error(), L.last_error()
    with pytest.raises(RuntimeError):
        L.vae_split_plan(*args)
