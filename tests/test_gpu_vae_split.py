"""-m gpu: the exact spatial split of the VAE decode (svi_vae_decode_part, WanVideoVAE.decode(split=...)) against the whole decode and the oracle.

A part runs conv2 / conv1 / middle on the whole latent frame, crops to its owned rectangle plus the planner's halo and runs the upsampling
stages and the head on the crop.  A cropped shape may select another convolution kernel family than the whole frame, so the bound between the
split and the whole decode is the one the project holds between its families (tests/test_gpu_vae.py: rel-L2 < 5e-6, max-abs < 5e-5), not bit
identity; against the oracle the file's usual 2e-5 / 2e-4."""
import numpy as np
import pytest
import torch

import synth
from gpu_util import errs, report
from oracle import wan_vae_oracle as wvo

pytestmark = pytest.mark.gpu

REL, MAXABS = 5e-6, 5e-5
BAND = 16                                   # pixels on either side of a cut
CASES = [("32x40_1x2", 701, (16, 3, 32, 40), (1, 2)), ("32x40_2x1", 701, (16, 3, 32, 40), (2, 1)), ("32x40_2x2", 701, (16, 3, 32, 40), (2, 2)),
         ("29x37_2x2", 702, (16, 2, 29, 37), (2, 2))]


@pytest.fixture(scope="module")
def vae():
    import svi_hip
    sd = {k: torch.from_numpy(v) for k, v in synth.vae_state_dict(500).items()}
    return svi_hip.WanVideoVAE.from_state_dict(sd), sd


_whole = {}


def whole_decode(v, seed, shape):
    """The latent and its unsplit decode, computed once per shape and shared (never written to)."""
    if (seed, shape) not in _whole:
        z = torch.from_numpy(synth.randn(seed, *shape)).cuda()
        _whole[(seed, shape)] = (z, v.decode([z], device="cuda")[0])
    return _whole[(seed, shape)]


def seam_band_maxabs(got, want, shape, split):
    """max |got - want| over the 16-pixel bands on either side of every cut (0 when the split has no cut)."""
    hh, ww = shape[2], shape[3]
    worst = 0.0
    for i in range(1, split[0]):
        y = 8 * (i * hh // split[0])
        worst = max(worst, float((got[:, :, y - BAND:y + BAND] - want[:, :, y - BAND:y + BAND]).abs().max()))
    for j in range(1, split[1]):
        x = 8 * (j * ww // split[1])
        worst = max(worst, float((got[..., x - BAND:x + BAND] - want[..., x - BAND:x + BAND]).abs().max()))
    return worst


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_assembled_split_decode_matches_whole_decode(vae, case):
    """(32, 40): every cut is more than 13 latent pixels from both borders, so the full halo is cropped and trimmed at every stage;
    (29, 37): odd sizes, unequal parts, halos clamped by the border.  The seam bands are held to the max-abs bound on their own, so that a seam
    error cannot hide in the whole-frame norm."""
    v, _ = vae
    name, seed, shape, split = case
    z, want = whole_decode(v, seed, shape)
    got = v.decode([z], device="cuda", split=split)[0]
    assert got.shape == want.shape and torch.isfinite(got).all()
    r, mx, _ = errs(got, want)
    band = seam_band_maxabs(got, want, shape, split)
    report("vae_split_vs_whole", case=name, rel_l2=r, max_abs=mx, seam_band_max_abs=band, identical=bool(torch.equal(got, want)))
    print(f"{name}: rel-L2 {r:.3e} max-abs {mx:.3e} seam-band max-abs {band:.3e}")
    assert r < REL and mx < MAXABS, (r, mx)
    assert band < MAXABS, band


_oracle = {}


def oracle_decode(sd, z, seed, shape):
    """The CPU oracle's decode, once per latent (the three splits of the first latent share one; ~10-20 s each, the slow part of this file)."""
    if (seed, shape) not in _oracle:
        with torch.no_grad():
            _oracle[(seed, shape)] = wvo.vae_decode(sd, z.cpu()[None])[0]
    return _oracle[(seed, shape)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_assembled_split_decode_matches_oracle(vae, case):
    v, sd = vae
    name, seed, shape, split = case
    z, _ = whole_decode(v, seed, shape)
    got = v.decode([z], device="cuda", split=split)[0]
    want = oracle_decode(sd, z, seed, shape)
    r, mx, _ = errs(got, want)
    report("vae_split_vs_oracle", case=name, rel_l2=r, max_abs=mx)
    print(f"{name}: vs oracle rel-L2 {r:.3e} max-abs {mx:.3e}")
    assert r < 2e-5 and mx < 2e-4, (r, mx)


def test_a_short_halo_shows_in_the_seam_bands(vae):
    """The seam check can fail: the same parts decoded with the stage 0 halo 6 latent pixels short (7 instead of 13; the later stages' rectangles
    as planned) break the seam-band bound of the test above."""
    v, _ = vae
    _, seed, shape, split = CASES[2]
    z, want = whole_decode(v, seed, shape)
    got = torch.empty_like(want)
    for p in range(split[0] * split[1]):
        v.decode_part(z, split, p, out=got, _short_halo=6)
    band = seam_band_maxabs(got, want, shape, split)
    report("vae_split_short_halo", reduction=6, seam_band_max_abs=band)
    print(f"short halo (13 - 6): seam-band max-abs {band:.3e}")
    assert torch.isfinite(got).all()
    assert band >= MAXABS, band


def test_part_writes_only_its_window(vae):
    """decode_part into a full frame filled with a sentinel leaves everything outside the owned window alone; a tight buffer holds the same values."""
    from svi_hip import _lib as L
    v, _ = vae
    _, seed, shape, split = CASES[3]
    z, want = whole_decode(v, seed, shape)
    for p in range(4):
        h0, h1, w0, w1 = (8 * a for a in L.vae_split_plan(shape[2], shape[3], *split, p)["owned"])
        full = torch.full_like(want, 7.5)
        assert v.decode_part(z, split, p, out=full) is full
        inside = torch.zeros(want.shape[2:], dtype=torch.bool, device="cuda")
        inside[h0:h1, w0:w1] = True
        assert bool((full[:, :, ~inside] == 7.5).all())
        assert float(full[:, :, inside].abs().max()) <= 1.0
        tight = v.decode_part(z, split, p)
        assert tuple(tight.shape) == (3, want.shape[1], h1 - h0, w1 - w0)
        assert torch.equal(tight, full[:, :, h0:h1, w0:w1])
        padded = torch.full((3, want.shape[1], h1 - h0 + 3, w1 - w0 + 5), 7.5, device="cuda")      # an all-gather buffer wider than the part
        v.decode_part(z, split, p, out=padded)
        assert torch.equal(padded[:, :, :h1 - h0, :w1 - w0], tight)
        assert bool((padded[:, :, h1 - h0:] == 7.5).all()) and bool((padded[:, :, :, w1 - w0:] == 7.5).all())


def test_one_part_is_todays_decode(vae):
    v, _ = vae
    z, want = whole_decode(v, 703, (16, 2, 5, 7))
    assert torch.equal(v.decode([z], device="cuda", split=(1, 1))[0], want)
    assert torch.equal(v.decode_part(z, (1, 1), 0), want)


def test_one_part_at_other_pitches_is_the_whole_decode(vae):
    """One part into a buffer 3 rows and 5 columns larger than the frame: the pitches are not the frame's, so the call runs the part form of
    the decoder walk (trivial plan: every stage's rectangle is the whole activation) instead of handing over to the whole decode, and must
    give the whole decode's bits; nothing outside the window is written."""
    v, _ = vae
    z, want = whole_decode(v, 703, (16, 2, 5, 7))
    H, W = want.shape[2:]
    padded = torch.full((3, want.shape[1], H + 3, W + 5), 7.5, device="cuda")
    assert v.decode_part(z, (1, 1), 0, out=padded) is padded
    assert torch.equal(padded[:, :, :H, :W], want)
    assert bool((padded[:, :, H:] == 7.5).all()) and bool((padded[:, :, :, W:] == 7.5).all())


def test_refusals(vae):
    v, _ = vae
    z, _ = whole_decode(v, 703, (16, 2, 5, 7))
    with pytest.raises(ValueError, match="tiled"):
        v.decode([z], device="cuda", tiled=True, split=(1, 2))
    with pytest.raises(RuntimeError, match="without a pixel"):
        v.decode([z], device="cuda", split=(1, 8))
    with pytest.raises(RuntimeError, match="outside"):
        v.decode_part(z, (1, 2), 2)


def _two_rank_worker(rank, world, port, queue):
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import svi_hip
        torch.cuda.set_device(0)
        v = svi_hip.WanVideoVAE.from_state_dict({k: torch.from_numpy(a) for k, a in synth.vae_state_dict(500).items()})
        z = torch.from_numpy(synth.randn(704, 16, 2, 16, 32)).cuda()
        whole = v.decode([z], device="cuda")[0]
        refused = False
        try:
            v.decode([z], device="cuda", split=(2, 2), group=dist.group.WORLD)       # four parts, two ranks: refused before any collective
        except ValueError as ex:
            refused = "needs a group of 4 ranks" in str(ex)
        got = v.decode([z], device="cuda", split=(1, 2), group=dist.group.WORLD)[0]
        r, mx, _ = errs(got, whole)
        # both ranks hold the same assembled video: compare checksums of the bits across the ranks
        mine = torch.tensor([float(got.double().sum()), float(got.double().abs().sum())], dtype=torch.float64)
        both = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(both, mine)
        same = all(torch.equal(b, both[0]) for b in both)
        gathered = [torch.empty(got.shape, dtype=torch.float32) for _ in range(world)]
        dist.all_gather(gathered, got.cpu())
        same = same and all(torch.equal(g, gathered[0]) for g in gathered)
        queue.put((rank, r, mx, bool(refused), bool(same)))
    finally:
        dist.destroy_process_group()


def test_two_ranks_over_gloo():
    """Two gloo ranks on the one GPU, fresh child processes: decode(split=(1, 2), group=world) on (16, 2, 16, 32) — each rank decodes its half into
    a tight buffer, one all-gather assembles the frame on both; a group whose size does not match the split is refused before any collective."""
    from spawn_util import run_ranks
    res = run_ranks(_two_rank_worker, 2, timeout=300)
    report("vae_split_two_ranks", ranks=[list(r) for r in sorted(res)])
    print(sorted(res))
    assert sorted(r[0] for r in res) == [0, 1], res
    assert all(r[3] for r in res), res                           # the 2 x 2 split on two ranks was refused
    assert all(r[4] for r in res), res                           # the same video on both ranks
    assert all(r[1] < REL and r[2] < MAXABS for r in res), res


def test_stream_loop_with_a_split_decode():
    """StreamLoop, tiny I2V synth model, 2 clips of 2 steps, vae_split=(1, 2) in local mode: 8-bit frames within 1 code value of the unsplit stream's
    (equality is expected almost everywhere; an 8-bit rounding boundary can flip within the fp32 bound)."""
    import svi_hip
    from gpu_util import dev
    c = synth.TINY_DIT_I2V
    sd = {k: torch.from_numpy(a) for k, a in synth.dit_state_dict(200, **c).items()}
    dit = svi_hip.WanDiT.from_state_dict(sd, eps=1e-6, num_heads=synth.num_heads_of(c), **c)
    v = svi_hip.WanVideoVAE.from_state_dict({k: torch.from_numpy(a) for k, a in synth.vae_state_dict(500).items()})
    H, W, NF, STEPS, CLIPS = 32, 48, 9, 2, 2
    img = torch.from_numpy(synth.condition_frames(31, 1, H, W))
    ref = torch.from_numpy(synth.condition_frames(32, 1, H, W)[0])
    prompts = [(dev(synth.text_context(40, 16, c["text_dim"], 9)), dev(synth.text_context(50, 16, c["text_dim"], 5)))]
    clipf = dev(synth.randn(33, 1, 257, 1280))
    kw = dict(clip_encoder=lambda first: clipf, num_motion_frames=1, num_frames=NF, num_inference_steps=STEPS, ref_pad_num=-1)
    plain = svi_hip.StreamLoop(dit, v, **kw).run(img, ref, prompts, CLIPS)
    split = svi_hip.StreamLoop(dit, v, vae_split=(1, 2), **kw).run(img, ref, prompts, CLIPS)
    assert split.dtype == torch.uint8 and split.shape == plain.shape
    diff = (split.int() - plain.int()).abs()
    n = int((diff > 0).sum())
    report("vae_split_stream", pixels=int(diff.numel()), differing=n, max_code_diff=int(diff.max()))
    print(f"stream: {n} of {diff.numel()} 8-bit values differ, max {int(diff.max())}")
    assert int(diff.max()) <= 1
    with pytest.raises(ValueError, match="tiled"):
        svi_hip.StreamLoop(dit, v, vae_split=(1, 2), tiled=True, **kw)
