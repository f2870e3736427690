"""The planner of the exact spatial split of the VAE encode (svi_vae_encode_split_plan; host arithmetic, no GPU).

A part owns a rectangle of the latent grid and runs conv1 and the four down stages on a crop of the video: at each of the five entry points
(video, entries of stages 0-3) the rectangle it needs is its owned rectangle, scaled, grown by what the layers between that point and the
encoder's middle block reach.  As for the decode, no numerical test can see a halo one pixel short with random weights, so the reach is
pinned here, structurally, against an independent walk of the parameter inventory."""
import ctypes as C

import pytest

from svi_hip import _lib as L
from svi_hip.vae import vae_param_shapes

GRIDS = [(60, 104), (20, 24), (29, 37), (7, 9), (32, 40)]
SPLITS = [(1, 2), (2, 1), (2, 2), (2, 4), (3, 1)]
FACTOR = (8, 8, 4, 2, 1)                     # pixels per latent pixel at the video and at the entries of stages 0-3


def walked_reaches():
    """(top/left, bottom/right) at the five entry points, from vae_param_shapes(): backwards from the entry of middle.0, the names in
    the order the encoder runs them.  A residual block adds the larger of its two convolutions in a row and its shortcut; a time_conv
    adds its spatial taps; a resample convolution (ZeroPad2d(0,1,0,1) + k x k stride 2: output o reads 2o .. 2o+k-1) turns a need of n
    into 2n on the top/left and 2n + k - 2 on the bottom/right; conv1 sits between the video and stage 0."""
    shapes = vae_param_shapes()
    e = "model.encoder."
    half = lambda name: max(shapes[name + ".weight"][-2:]) // 2 if name + ".weight" in shapes else 0      # noqa: E731
    blocks, idx = [], 0
    while any(k.startswith(f"{e}downsamples.{idx}.") for k in shapes):
        blocks.append(f"{e}downsamples.{idx}.")
        idx += 1
    tl = br = 0
    entries = []                                               # filled from stage 3 backwards
    for p in reversed(blocks):
        if p + "resample.1.weight" in shapes:
            entries.append((tl, br))                           # the entry of the stage behind this downsample block
            k = max(shapes[p + "resample.1.weight"][-2:])
            tl, br = tl + half(p + "time_conv"), br + half(p + "time_conv")
            tl, br = 2 * tl, 2 * br + k - 2
        else:
            n = max(half(p + "residual.2") + half(p + "residual.6"), half(p + "shortcut"))
            tl, br = tl + n, br + n
    entries.append((tl, br))                                   # stage 0
    n = half(e + "conv1")
    entries.append((tl + n, br + n))                           # video
    return entries[::-1]


def plans(grid, split):
    return [L.vae_encode_split_plan(*grid, *split, p) for p in range(split[0] * split[1])]


def test_reaches_follow_from_the_parameter_inventory():
    want = walked_reaches()
    assert want == [(61, 68), (60, 67), (28, 31), (12, 13), (4, 4)]          # the hand walk
    for grid in GRIDS:
        for split in SPLITS:
            for pl in plans(grid, split):
                assert pl["reach"] == want, (grid, split, pl)


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("split", SPLITS)
def test_owned_rectangles_tile_the_grid(grid, split):
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
    assert all(v == 1 for row in cover for v in row)


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("split", SPLITS)
def test_rectangles_hold_the_reach_keep_the_phase_and_stop_at_the_border(grid, split):
    hh, ww = grid
    reach = walked_reaches()
    for pl in plans(grid, split):
        own = pl["owned"]
        for k, r in enumerate(pl["rects"]):
            f, (tl, br) = FACTOR[k], reach[k]
            for lo, hi, o0, o1, full in ((r[0], r[1], own[0], own[1], hh), (r[2], r[3], own[2], own[3], ww)):
                assert 0 <= lo <= o0 * f and o1 * f <= hi <= full * f              # contains the owned rectangle, inside the image
                assert lo % f == 0                                                 # a multiple of 2^(3-s) entering stage s, of 8 in the video
                need = max(o0 * f - tl, 0)
                assert need - f < lo <= need                                       # the need, rounded up by less than one phase
                assert hi == min(o1 * f + br, full * f)
        # each entry point's rectangle contains what the next one needs (its rectangle before the origin is rounded down to the phase), grown by
        # what lies between the two and mapped through the stride-2 rule, wherever the border does not clamp it
        need_lo = lambda k, a: max(own[a] * FACTOR[k] - reach[k][0], 0)           # noqa: E731
        v, s0 = pl["rects"][0], pl["rects"][1]
        n = reach[0][0] - reach[1][0]                                              # conv1
        assert n == 1
        for a in (0, 2):
            full = (hh if a == 0 else ww) * 8
            assert v[a] <= max(need_lo(1, a) - n, 0) and v[a + 1] >= min(s0[a + 1] + n, full)
        for k in range(1, 4):
            q, r = pl["rects"][k], pl["rects"][k + 1]
            grow = reach[k][0] - 2 * reach[k + 1][0]                               # the two residual blocks of the stage
            assert grow == 4
            for a in (0, 2):
                full = (hh if a == 0 else ww) * FACTOR[k]
                # through the downsample block output o reads inputs 2o .. 2o+2; the stage's residual blocks sit in front of it
                assert q[a] <= max(2 * need_lo(k + 1, a) - grow, 0)
                assert q[a + 1] >= min(2 * (r[a + 1] - 1) + 3 + grow, full)
                # what the part computes from crop q covers r: [q0 / 2, q0 / 2 + (q1 - q0) // 2)
                assert q[a] % 2 == 0 and q[a] // 2 <= r[a] and r[a + 1] <= q[a] // 2 + (q[a + 1] - q[a]) // 2


def test_full_reach_is_exercised_away_from_the_border():
    """At (20, 24) in 2 x 2 (the GPU test's 160 x 192 video) both cuts are farther than 68 pixels from every border: every interior side
    extends by exactly the reach (the top/left rounded up to the phase), no border side extends."""
    reach = walked_reaches()
    for pl in plans((20, 24), (2, 2)):
        own = pl["owned"]
        for k, r in enumerate(pl["rects"]):
            f, (tl, br) = FACTOR[k], reach[k]
            up = -(-tl // f) * f
            assert (own[0] * f - r[0], r[1] - own[1] * f) == ((up, 0) if own[0] else (0, br))
            assert (own[2] * f - r[2], r[3] - own[3] * f) == ((up, 0) if own[2] else (0, br))


@pytest.mark.parametrize("grid", GRIDS)
def test_one_part_is_the_whole_frame_without_halo(grid):
    hh, ww = grid
    pl = L.vae_encode_split_plan(hh, ww, 1, 1, 0)
    assert pl["owned"] == (0, hh, 0, ww) and pl["reach"] == [(0, 0)] * 5
    assert pl["rects"] == [(0, hh * f, 0, ww * f) for f in FACTOR]


@pytest.mark.parametrize("args,word", [((7, 9, 2, 2, 4), "outside"), ((7, 9, 2, 2, -1), "outside"), ((7, 9, 8, 1, 0), "without a pixel"),
                                       ((7, 9, 1, 10, 0), "without a pixel"), ((7, 9, 0, 1, 0), "positive"), ((0, 9, 1, 1, 0), "positive")])
def test_bad_arguments_are_refused_with_a_message(args, word):
    out = (C.c_int32 * 34)()
    assert L.lib().svi_vae_encode_split_plan(*args, out) != 0
    assert word in L.last_error(), L.last_error()
    with pytest.raises(RuntimeError):
        L.vae_encode_split_plan(*args)
