"""The VAE's plane-fed convolution launches (host logic, no GPU): the frame-interleaved tile order the kernels walk, which kernel runs, and what
the 32-bit buffer descriptors must reach, at the video sizes and clip lengths the pipelines use.  Pure arithmetic behind the C ABI
(svi_vae_conv_plan, svi_vae_tile_order), the same functions launch_conv_planes and the kernels call."""
import pytest

from svi_hip import _lib as L

WINDOW = 0xFFE00000              # the activation descriptors' range (csrc/svi_vae.hip)
FRAMES = (1, 5, 9, 17, 21, 41, 81)
SIZES = [(480, 832), (832, 480), (480, 848), (720, 1280), (1280, 720), (512, 512), (256, 256), (488, 840)]      # (H, W); 488 x 840: no frame is whole tiles
# the residual-block (and head) convolutions of Wan's VAE, (Cin, Cout, spatial downscale of the video): decoder, then encoder
LAYERS = [(384, 384, 8), (192, 384, 4), (384, 384, 4), (192, 192, 2), (96, 96, 1), (96, 3, 1),
          (96, 96, 1), (96, 192, 2), (192, 192, 2), (192, 384, 4), (384, 384, 4), (384, 384, 8), (384, 32, 8)]


@pytest.fixture(autouse=True)
def clean_switches():
    yield
    for k in ("SVI_VAE_PAIR", "SVI_VAE_TILE_ORDER", "SVI_VAE_DMA"):
        L.set_switch(k, None)


def order_by_definition(T, Lf, G):
    """Groups of G tiles (the last one shorter when G does not divide Lf) walked through all T frames, group after group."""
    out = []
    for gbase in range(0, Lf, G):
        for t in range(T):
            out.extend(t * Lf + j for j in range(gbase, min(gbase + G, Lf)))
    return out


@pytest.mark.parametrize("T,Lf,G", [
    (81, 1560, 52),                       # C2 full resolution: T x G even
    (81, 1590, 53), (81, 3600, 45),       # 480 x 848 and portrait 720p: T x G odd
    (9, 12, 3),                           # latent 8 x 6 decoded to 64 x 48: T x G = 27
    (5, 10, 3), (9, 3, 2), (7, 13, 4),    # a last group shorter than G
    (4, 6, 6), (3, 5, 5),                 # G == Lf: one group
    (1, 7, 3), (1, 1, 1), (2, 1, 1),      # one frame, one tile per frame
])
def test_tile_order_is_a_permutation_and_follows_its_definition(T, Lf, G):
    got = L.vae_tile_order(T, Lf, G)
    assert len(got) == T * Lf
    assert sorted(got) == list(range(T * Lf))                 # every tile exactly once
    assert got == order_by_definition(T, Lf, G)


def test_tile_order_refuses_bad_arguments():
    for args in ((0, 4, 2), (3, 0, 1), (3, 4, 0), (3, 4, 5)):
        with pytest.raises(RuntimeError):
            L.vae_tile_order(*args)


@pytest.mark.parametrize("H,W", SIZES)
def test_every_plane_fed_descriptor_stays_inside_its_window(H, W):
    """Whatever kernel the launcher picks, the bytes its largest activation descriptor must address stay below the 0xFFE00000 window and
    inside the launch guard's (kt + 3)-frame bound — in particular for the two-tile kernel, whose tiles can lie a whole clip apart."""
    pairs = 0
    for Cin, Cout, down in LAYERS:
        for frames in FRAMES:
            p = L.vae_conv_plan(Cin, Cout, 3, frames, H // down, W // down)
            if p["kernel"] is None:
                continue
            pairs += p["kernel"] == "pair"
            where = (H, W, Cin, Cout, down, frames, p)
            assert p["desc_bytes"] < WINDOW, where
            assert p["desc_bytes"] <= p["guard_bytes"], where
    assert pairs > 0


@pytest.mark.parametrize("H,W,span", [(480, 832, 0), (832, 480, 0), (480, 848, 80), (1280, 720, 80), (720, 1280, 0)])
def test_pair_span_at_full_resolution(H, W, span):
    """The frame distance between the two tiles of a workgroup at 81 frames of full resolution (Cin = 96): none where groups hold an even number of
    tiles, the whole clip where T x G is odd (the last frame of one tile group and the first frame of the next) — a distance no single descriptor
    reaches (80 frames of 480 x 848 x 96 fp16 = 6.3 GB)."""
    p = L.vae_conv_plan(96, 96, 3, 81, H, W)
    assert p["kernel"] == "pair" and p["ord_T"] == 81
    assert (81 * p["ord_G"]) % 2 == (span == 80)
    assert p["pair_span"] == span, p
    assert p["desc_bytes"] < WINDOW


@pytest.mark.parametrize("T,Ho,Wo", [(9, 64, 48), (5, 32, 40), (3, 64, 48), (4, 48, 80), (9, 32, 24)])
def test_pair_span_matches_the_tile_order(T, Ho, Wo):
    """The planner's pair span against the frames of tiles 2p and 2p + 1 of the order itself."""
    p = L.vae_conv_plan(96, 96, 3, T, Ho, Wo)
    assert p["kernel"] == "pair" and p["ord_T"] == T
    order = L.vae_tile_order(p["ord_T"], p["ord_Lf"], p["ord_G"])
    want = max(abs(order[i + 1] // p["ord_Lf"] - order[i] // p["ord_Lf"]) for i in range(0, len(order) - 1, 2))
    assert p["pair_span"] == want
    assert p["workgroups"] == (len(order) + 1) // 2


def test_c2_plan_is_pinned_and_follows_the_switches():
    """The headline size (81 frames of 480 x 832, the full-resolution convolutions): the two-tile kernel on the frame-interleaved order with groups of
    52 tiles.  SVI_VAE_PAIR=0: the one-tile kernel on the same order.  SVI_VAE_TILE_ORDER=0: tiles in pixel order (pairs of neighbours).
    SVI_VAE_DMA=0: the layer does not take fp16 planes."""
    want = dict(kernel="pair", ord_T=81, ord_Lf=1560, ord_G=52, workgroups=81 * 1560 // 2, pair_span=0)
    p = L.vae_conv_plan(96, 96, 3, 81, 480, 832)
    assert {k: p[k] for k in want} == want, p
    assert L.vae_conv_plan(96, 3, 3, 81, 480, 832)["kernel"] == "dma2h<1>"                  # the decoder's head: one 32-channel block
    assert L.vae_conv_plan(384, 384, 3, 21, 60, 104)["ord_T"] == 0                          # 6240 pixels per frame: not whole tiles
    assert L.vae_conv_plan(96, 96, 3, 1, 480, 832)["ord_T"] == 0                            # one frame
    assert L.vae_conv_plan(96, 96, 1, 81, 480, 832)["ord_T"] == 0                           # no earlier frames to reuse
    assert L.vae_conv_plan(16, 384, 3, 21, 60, 104)["kernel"] is None                       # Cin not a multiple of 32
    L.set_switch("SVI_VAE_PAIR", 0)
    p = L.vae_conv_plan(96, 96, 3, 81, 480, 832)
    assert (p["kernel"], p["ord_T"], p["ord_G"], p["workgroups"], p["pair_span"]) == ("dma2h<3>", 81, 52, 81 * 1560, 0)
    L.set_switch("SVI_VAE_PAIR", None)
    L.set_switch("SVI_VAE_TILE_ORDER", 0)
    p = L.vae_conv_plan(96, 96, 3, 81, 480, 832)
    assert (p["kernel"], p["ord_T"], p["workgroups"], p["pair_span"]) == ("pair", 0, 81 * 1560 // 2, 0)
    L.set_switch("SVI_VAE_TILE_ORDER", None)
    L.set_switch("SVI_VAE_DMA", 0)
    assert L.vae_conv_plan(96, 96, 3, 81, 480, 832)["kernel"] is None
