"""-m gpu: the HIP VAE (whole clip resident, fp32 MFMA implicit-GEMM convs) against the reference's chunked/cached
implementation (golden vectors) and against the oracle on further shapes.

fp32 in, fp32 out, exact-fp32 MFMA: the only difference is summation order -> rel-L2 <= 2e-5, max-abs <= 2e-4
(the decoder output lies in [-1,1])."""
import numpy as np
import pytest
import torch

import synth
from gpu_util import errs, report
from oracle import wan_vae_oracle as wvo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vae():
    import svi_hip
    sd = {k: torch.from_numpy(v) for k, v in synth.vae_state_dict(500).items()}
    return svi_hip.WanVideoVAE.from_state_dict(sd), sd


@pytest.mark.parametrize("key,seed,shape", [("decode_3f", 501, (16, 3, 4, 6)), ("decode_1f", 502, (16, 1, 4, 6)),
                                            ("decode_2f_tinyhw", 505, (16, 2, 2, 2))])
def test_decode_matches_reference(vae, golden, key, seed, shape):
    v, _ = vae
    g = golden("vae.npz")
    z = torch.from_numpy(synth.randn(seed, 1, *shape))[0]
    out = v.decode([z.cuda()], device="cuda")[0]
    r, mx, _ = errs(out, g[key])
    report("vae_decode", case=key, rel_l2=r, max_abs=mx)
    assert out.shape == g[key].shape
    assert r < 2e-5 and mx < 2e-4, (r, mx)


@pytest.mark.parametrize("key,seed,shape", [("encode_9f", 503, (3, 9, 32, 48)), ("encode_1f", 504, (3, 1, 32, 48))])
def test_encode_matches_reference(vae, golden, key, seed, shape):
    v, _ = vae
    g = golden("vae.npz")
    vid = torch.from_numpy(np.tanh(synth.randn(seed, *shape)))
    out = v.encode([vid.cuda()], device="cuda")[0]
    r, mx, _ = errs(out, g[key])
    report("vae_encode", case=key, rel_l2=r, max_abs=mx)
    assert out.shape == g[key].shape
    assert r < 2e-5 and mx < 2e-4, (r, mx)


def test_decode_encode_vs_oracle_more_shapes(vae):
    """Odd spatial sizes (pixel tiles that straddle rows/frames), 5 latent frames (both temporal upsamples fire twice)."""
    v, sd = vae
    with torch.no_grad():
        z = torch.from_numpy(synth.randn(601, 1, 16, 5, 3, 5))
        want = wvo.vae_decode(sd, z)[0]
        got = v.decode([z[0].cuda()], device="cuda")[0]
        r, mx, _ = errs(got, want)
        report("vae_decode_oracle", rel_l2=r, max_abs=mx)
        assert r < 2e-5 and mx < 2e-4, (r, mx)
        vid = torch.from_numpy(np.tanh(synth.randn(602, 1, 3, 13, 24, 40)))
        want = wvo.vae_encode(sd, vid)[0]
        got = v.encode([vid[0].cuda()], device="cuda")[0]
        r, mx, _ = errs(got, want)
        report("vae_encode_oracle", rel_l2=r, max_abs=mx)
        assert r < 2e-5 and mx < 2e-4, (r, mx)


def test_frame_causality(vae):
    """Size-independent property of the causal VAE: decoded frames 0..4k depend only on latent frames 0..k."""
    v, _ = vae
    z = torch.from_numpy(synth.randn(611, 16, 4, 3, 3)).cuda()
    full = v.decode([z], device="cuda")[0]
    part = v.decode([z[:, :2].contiguous()], device="cuda")[0]
    assert torch.allclose(full[:, :5], part, atol=1e-5, rtol=0)


def test_batch_of_clips_and_tiled_path(vae):
    v, sd = vae
    zs = [torch.from_numpy(synth.randn(620 + i, 16, 2, 4, 4)).cuda() for i in range(2)]
    both = v.decode(zs, device="cuda")
    for i in range(2):
        assert torch.equal(both[i], v.decode([zs[i]], device="cuda")[0])


@pytest.mark.parametrize("case", synth.TILED_DECODE_CASES, ids=lambda c: c[0])
def test_tiled_decode_matches_reference(vae, golden, case):
    """Row a21: WanVideoVAE.decode(tiled=True) = tiled_decode (vae:643-693) against the reference's own output: 3x3 tiles and a
    ragged grid with clipped tiles; latents at twice unit scale so that 1.2 % of the pixels sit on the clamp (the reference clamps
    AFTER blending un-clamped tiles)."""
    v, _ = vae
    name, zshape, size, stride, seed = case
    want = golden("vae_tiled.npz")["decode_" + name]
    z = torch.from_numpy(2.0 * synth.randn(seed, *zshape)).cuda()
    got = v.decode([z], device="cuda", tiled=True, tile_size=size, tile_stride=stride)[0]
    r, mx, _ = errs(got, want)
    report("vae_tiled_decode", case=name, rel_l2=r, max_abs=mx)
    assert got.shape == want.shape and r < 2e-5 and mx < 2e-4, (r, mx)
    assert float(got.abs().max()) <= 1.0


@pytest.mark.parametrize("case", synth.TILED_ENCODE_CASES, ids=lambda c: c[0])
def test_tiled_encode_matches_reference(vae, golden, case):
    v, _ = vae
    name, vshape, size, stride, seed = case
    g = golden("vae_tiled.npz")
    vid = torch.from_numpy(np.tanh(synth.randn(seed, *vshape))).cuda()
    got = v.encode([vid], device="cuda", tiled=True, tile_size=size, tile_stride=stride)[0]
    r, mx, _ = errs(got, g["encode_" + name])
    report("vae_tiled_encode", case=name, rel_l2=r, max_abs=mx)
    assert r < 2e-5 and mx < 2e-4, (r, mx)
    # a batch: the reference multiplies tile_size by 8 inside its per-video loop (vae:765-767), so the second video of a batch is
    # encoded with tiles 8x larger again — here one tile = the un-tiled encode.  Pinned as observable behaviour.
    both = v.encode([vid, vid], device="cuda", tiled=True, tile_size=size, tile_stride=stride)
    r0 = errs(both[0], g["encode_" + name])[0]
    r1 = errs(both[1], g["encode_" + name + "_batch_second"])[0]
    assert r0 < 2e-5 and r1 < 2e-5, (r0, r1)
    assert torch.equal(both[1], v.encode([vid], device="cuda")[0])


def test_tiled_blend_is_the_reference_arithmetic(vae):
    """The blend alone, bit for bit: tiles decoded un-tiled by the HIP VAE itself (clamped output is NOT what is blended, so use
    latents small enough that nothing clamps), masks / accumulation / division restated on the host in the reference's order."""
    from oracle import wan_vae_oracle as wvo
    v, _ = vae
    z = torch.from_numpy(0.05 * synth.randn(640, 16, 1, 7, 9)).cuda()
    size, stride = (4, 4), (3, 2)
    got = v.decode([z], device="cuda", tiled=True, tile_size=size, tile_stride=stride)[0].cpu()

    def dec(t):
        out = v.decode([t[0].contiguous().cuda()], device="cuda").cpu()
        assert float(out.abs().max()) < 1.0
        return out
    want = wvo._blend(dec, z.cpu()[None], (1, 3, 1, 56, 72), size, stride, lambda a: a * 8,
                      ((size[0] - stride[0]) * 8, (size[1] - stride[1]) * 8)).clamp(-1, 1)[0]
    assert torch.equal(got, want)


@pytest.mark.parametrize("switch", ["SVI_VAE_X2H", "SVI_VAE_EXACT_FP32"])
def test_every_convolution_family_meets_the_same_bounds(vae, golden, switch):
    """Default: the fp16 two-term convolution wherever the producer (RMS_norm [+ SiLU]) bounds the input, the bf16 three-term one
    elsewhere.  SVI_VAE_X2H=0 sends everything to the three-term kernel, SVI_VAE_EXACT_FP32=1 to the fp32 MFMA kernel: the three hold
    the same parity bounds against the reference, and the default differs from the other two far below them."""
    from svi_hip import _lib
    v, _ = vae
    g = golden("vae.npz")
    z = torch.from_numpy(synth.randn(501, 1, 16, 3, 4, 6))[0].cuda()
    vid = torch.from_numpy(np.tanh(synth.randn(503, 3, 9, 32, 48))).cuda()
    dflt_d, dflt_e = v.decode([z], device="cuda")[0], v.encode([vid], device="cuda")[0]
    try:
        _lib.set_switch(switch, "0" if switch == "SVI_VAE_X2H" else "1")
        alt_d, alt_e = v.decode([z], device="cuda")[0], v.encode([vid], device="cuda")[0]
    finally:
        _lib.set_switch(switch, None)
    for out, key in ((alt_d, "decode_3f"), (alt_e, "encode_9f")):
        r, mx, _ = errs(out, g[key])
        assert r < 2e-5 and mx < 2e-4, (switch, key, r, mx)
    rd, re = errs(dflt_d, alt_d)[0], errs(dflt_e, alt_e)[0]
    report("vae_conv_families", switch=switch, decode_default_vs_alt=rd, encode_default_vs_alt=re, identical=bool(torch.equal(dflt_d, alt_d)))
    assert rd < 5e-6 and re < 5e-6, (rd, re)
    assert not torch.equal(dflt_d, alt_d)                 # the default really took another kernel


def test_gain_vector_with_a_dead_channel_keeps_the_three_term_kernel(golden):
    """The static activation bound needs gains of comparable size: a norm whose gamma has a zero channel must not send its consumer to
    the fp16 kernel (that channel's activations would be subnormal after the common scale).  Result: still within the bounds of the
    oracle run on the same weights."""
    import svi_hip
    sd = {k: torch.from_numpy(v.copy()) for k, v in synth.vae_state_dict(500).items()}
    k = "model.decoder.middle.0.residual.0.gamma"
    sd[k][3] = 0.0
    sd[k][7] = 1e-5
    v = svi_hip.WanVideoVAE.from_state_dict(sd)
    z = torch.from_numpy(synth.randn(501, 1, 16, 3, 4, 6))[0]
    out = v.decode([z.cuda()], device="cuda")[0]
    with torch.no_grad():
        want = wvo.vae_decode(sd, z[None])[0]
    r, mx, _ = errs(out, want)
    report("vae_dead_gain_channel", rel_l2=r, max_abs=mx)
    assert r < 2e-5 and mx < 2e-4, (r, mx)


@pytest.mark.parametrize("shape", [(16, 3, 12, 20), (16, 2, 30, 52), (16, 2, 5, 3)])
def test_plane_fed_convolutions_agree_with_the_on_the_fly_split(vae, shape):
    """Residual-block convolutions fed by the producing RMS_norm's fp16 word pairs through LDS-DMA with the three x-taps of a kernel row
    served from one staged strip (conv_dma2h_kernel, the default) against the same convolutions splitting their fp32 input on the fly
    (SVI_VAE_DMA=0, conv_igemm_x3_kernel<true>): the same products, another summation order (x-taps innermost) — decode and encode agree
    to fp32 rounding (rel-L2 <= 5e-6, max-abs <= 5e-5 on outputs of unit scale), borders, causal padding, the hidden first frame of the
    upsampling time convolutions, ragged pixel tiles and strips that run across image rows and frames included (widths 24 .. 416 px, not
    multiples of the 256-pixel tile)."""
    from svi_hip import _lib as L
    v, _ = vae
    z = torch.from_numpy(synth.randn(611, *shape)).cuda()
    vid = torch.from_numpy(np.tanh(synth.randn(612, 3, 4 * (shape[1] - 1) + 1, 8 * shape[2], 8 * shape[3]))).cuda()
    a_dec, a_enc = v.decode([z], device="cuda")[0], v.encode([vid], device="cuda")[0]
    L.set_switch("SVI_VAE_DMA", 0)
    try:
        b_dec, b_enc = v.decode([z], device="cuda")[0], v.encode([vid], device="cuda")[0]
    finally:
        L.set_switch("SVI_VAE_DMA", None)
    assert torch.isfinite(a_dec).all() and torch.isfinite(a_enc).all()
    rd, md, _ = errs(a_dec, b_dec)
    re, me, _ = errs(a_enc, b_enc)
    report("vae_dma_vs_on_the_fly", shape=list(shape), decode_rel=rd, decode_maxabs=md, encode_rel=re, encode_maxabs=me)
    assert rd < 5e-6 and md < 5e-5 and re < 5e-6 and me < 5e-5, (rd, md, re, me)


@pytest.mark.parametrize("shape", [(16, 3, 12, 20), (16, 2, 30, 52), (16, 2, 5, 3), (16, 1, 7, 9), (16, 4, 30, 52), (16, 3, 8, 6), (16, 2, 4, 5)])
def test_two_tiles_per_workgroup_give_the_one_tile_kernels_bits(vae, shape):
    """conv_dma2h_pair_kernel (round 6, the default: two 256-pixel tiles per workgroup share every K step's weights) against conv_dma2h_kernel<3>
    (SVI_VAE_PAIR=0): the same products in the same order per pixel — decode and encode bit for bit, on grids with an odd number of tiles (the pair's second
    tile lies past the end), tiles that straddle image rows and frames, one frame, and the frame-interleaved tile order (whole tiles per frame: 30 x 52 latent
    = 240 x 416 px = 390 tiles per frame).  8 x 6 latent: 64 x 48 px = 12 tiles per frame in groups of 3 over 9 frames — 27 tiles per group, so pairs join
    the last frame of one group to the first frame of the next (svi_vae_conv_plan's pair span: 8 frames); at 32 x 24 px 3 tiles per frame in groups of 2
    (a last group of one).  4 x 5 latent: 32 x 40 px = 5 tiles per frame in groups of 3 (a shorter last group), 5 frames."""
    from svi_hip import _lib as L
    v, _ = vae
    z = torch.from_numpy(synth.randn(621, *shape)).cuda()
    vid = torch.from_numpy(np.tanh(synth.randn(622, 3, 4 * (shape[1] - 1) + 1, 8 * shape[2], 8 * shape[3]))).cuda()
    a_dec, a_enc = v.decode([z], device="cuda")[0], v.encode([vid], device="cuda")[0]
    L.set_switch("SVI_VAE_PAIR", 0)
    try:
        b_dec, b_enc = v.decode([z], device="cuda")[0], v.encode([vid], device="cuda")[0]
    finally:
        L.set_switch("SVI_VAE_PAIR", None)
    assert torch.isfinite(a_dec).all() and torch.isfinite(a_enc).all()
    assert torch.equal(a_dec, b_dec) and torch.equal(a_enc, b_enc)


@pytest.mark.parametrize("shape", [(16, 3, 12, 20), (16, 2, 30, 52), (16, 2, 5, 3), (16, 1, 7, 9)])
def test_upsample_convolution_phases_agree_with_the_nine_tap_form(vae, shape):
    """The convolution behind a nearest x2 upsample (Resample upsample2d/3d, vae:120-131) as four 2x2 convolutions of the small image with
    pre-summed kernels (the default) against the one 3x3 convolution reading through the upsample (SVI_VAE_UP_PHASES=0): the same sum with
    the kernel entries that meet one input pixel added beforehand — decode agrees to fp32 rounding (rel-L2 <= 5e-6, max-abs <= 5e-5), image
    borders (where the upsampled image's zero padding is the small image's), odd sizes and single frames included."""
    from svi_hip import _lib as L
    v, _ = vae
    z = torch.from_numpy(synth.randn(613, *shape)).cuda()
    a = v.decode([z], device="cuda")[0]
    L.set_switch("SVI_VAE_UP_PHASES", 0)
    try:
        b = v.decode([z], device="cuda")[0]
    finally:
        L.set_switch("SVI_VAE_UP_PHASES", None)
    assert torch.isfinite(a).all()
    r, mx, _ = errs(a, b)
    report("vae_upsample_phases_vs_nine_taps", shape=list(shape), decode_rel=r, decode_maxabs=mx)
    assert r < 5e-6 and mx < 5e-5, (r, mx)


def test_pair_tile_order_shape_vs_oracle(vae):
    """The default decode and encode at the latent 8 x 6 of the pair test above (64 x 48 px, 9 frames: tile groups whose pairs span the clip) against
    the oracle, within the file's bounds."""
    v, sd = vae
    with torch.no_grad():
        z = torch.from_numpy(synth.randn(631, 1, 16, 3, 8, 6))
        want = wvo.vae_decode(sd, z)[0]
        got = v.decode([z[0].cuda()], device="cuda")[0]
        r, mx, _ = errs(got, want)
        vid = torch.from_numpy(np.tanh(synth.randn(632, 1, 3, 9, 64, 48)))
        want_e = wvo.vae_encode(sd, vid)[0]
        got_e = v.encode([vid[0].cuda()], device="cuda")[0]
        re, me, _ = errs(got_e, want_e)
    report("vae_pair_order_oracle", decode_rel=r, decode_maxabs=mx, encode_rel=re, encode_maxabs=me)
    assert got.shape == want.shape and got_e.shape == want_e.shape
    assert r < 2e-5 and mx < 2e-4, (r, mx)
    assert re < 2e-5 and me < 2e-4, (re, me)
