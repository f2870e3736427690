"""-m gpu: the exact spatial split of the VAE encode (svi_vae_encode_part / svi_vae_encode_tail, WanVideoVAE.encode(split=...)) against the whole
encode and the oracle.

A part runs conv1 and the four down stages on a crop of the video (its owned rectangle plus the planner's halo, trimmed after every downsample
block) and writes its owned window of the feature map entering the encoder's middle block; the middle block, the head and model.conv1 run on
the assembled map.  A cropped shape may select another convolution kernel family than the whole frame, so the bound between the split and the
whole encode is the one the project holds between its families (tests/test_gpu_vae.py: rel-L2 < 5e-6, max-abs < 5e-5), not bit identity;
against the oracle the file's usual 2e-5 / 2e-4."""
import numpy as np
import pytest
import torch

import synth
from gpu_util import errs, report
from oracle import wan_vae_oracle as wvo

pytestmark = pytest.mark.gpu

REL, MAXABS = 5e-6, 5e-5
BAND = 4                                    # latent pixels on either side of a cut
FULL, ODD = (3, 5, 160, 192), (3, 5, 232, 296)
CASES = [("160x192_1x2", 711, FULL, (1, 2)), ("160x192_2x1", 711, FULL, (2, 1)), ("160x192_2x2", 711, FULL, (2, 2)), ("232x296_2x2", 712, ODD, (2, 2))]


@pytest.fixture(scope="module")
def vae():
    import svi_hip
    sd = {k: torch.from_numpy(v) for k, v in synth.vae_state_dict(500).items()}
    return svi_hip.WanVideoVAE.from_state_dict(sd), sd


_whole = {}


def whole_encode(v, seed, shape):
    """The video and its unsplit encode, computed once per shape and shared (never written to)."""
    if (seed, shape) not in _whole:
        vid = torch.from_numpy(np.tanh(synth.randn(seed, *shape))).cuda()
        _whole[(seed, shape)] = (vid, v.encode([vid], device="cuda")[0])
    return _whole[(seed, shape)]


def seam_band_maxabs(got, want, shape, split):
    """max |got - want| over the 4 latent pixels on either side of every cut (0 when the split has no cut)."""
    hh, ww = shape[2] // 8, shape[3] // 8
    worst = 0.0
    for i in range(1, split[0]):
        y = i * hh // split[0]
        worst = max(worst, float((got[:, :, y - BAND:y + BAND] - want[:, :, y - BAND:y + BAND]).abs().max()))
    for j in range(1, split[1]):
        x = j * ww // split[1]
        worst = max(worst, float((got[..., x - BAND:x + BAND] - want[..., x - BAND:x + BAND]).abs().max()))
    return worst


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_assembled_split_encode_matches_whole_encode(vae, case):
    """(160, 192): every cut is more than 68 px from both borders, so the full halo is cropped and trimmed at every stage; (232, 296): an odd
    29 x 37 grid, unequal parts, halos clamped by the border.  The seam bands are held to the max-abs bound on their own, so that a seam error
    cannot hide in the whole-frame norm."""
    v, _ = vae
    name, seed, shape, split = case
    vid, want = whole_encode(v, seed, shape)
    got = v.encode([vid], device="cuda", split=split)[0]
    assert got.shape == want.shape and torch.isfinite(got).all()
    r, mx, _ = errs(got, want)
    band = seam_band_maxabs(got, want, shape, split)
    report("vae_encode_split_vs_whole", case=name, rel_l2=r, max_abs=mx, seam_band_max_abs=band, identical=bool(torch.equal(got, want)))
    print(f"{name}: rel-L2 {r:.3e} max-abs {mx:.3e} seam-band max-abs {band:.3e}")
    assert r < REL and mx < MAXABS, (r, mx)
    assert band < MAXABS, band


_oracle = {}


def oracle_encode(sd, vid, seed, shape):
    """The CPU oracle's encode, once per video (the three splits of the first video share one)."""
    if (seed, shape) not in _oracle:
        with torch.no_grad():
            _oracle[(seed, shape)] = wvo.vae_encode(sd, vid.cpu()[None])[0]
    return _oracle[(seed, shape)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_assembled_split_encode_matches_oracle(vae, case):
    v, sd = vae
    name, seed, shape, split = case
    vid, _ = whole_encode(v, seed, shape)
    got = v.encode([vid], device="cuda", split=split)[0]
    want = oracle_encode(sd, vid, seed, shape)
    r, mx, _ = errs(got, want)
    report("vae_encode_split_vs_oracle", case=name, rel_l2=r, max_abs=mx)
    print(f"{name}: vs oracle rel-L2 {r:.3e} max-abs {mx:.3e}")
    assert r < 2e-5 and mx < 2e-4, (r, mx)


def test_a_short_halo_shows_in_the_seam_bands(vae):
    """The seam check can fail: the same parts encoded with only 8 video pixels of halo (1 latent pixel instead of 61 / 68 video pixels; the
    later rectangles shrink with it) break the seam-band bound of the test above."""
    v, _ = vae
    _, seed, shape, split = CASES[2]
    vid, want = whole_encode(v, seed, shape)
    feat = torch.empty((want.shape[1], shape[2] // 8, shape[3] // 8, 384), device="cuda")
    for p in range(split[0] * split[1]):
        v.encode_part(vid, split, p, out=feat, _short_halo=8)
    got = v.encode_tail(feat)
    band = seam_band_maxabs(got, want, shape, split)
    report("vae_encode_split_short_halo", halo_px=8, seam_band_max_abs=band)
    print(f"short halo (8 px): seam-band max-abs {band:.3e}")
    assert torch.isfinite(got).all()
    assert band >= MAXABS, band


def test_part_writes_only_its_window(vae):
    """encode_part into a full-frame feature buffer filled with a sentinel leaves everything outside the owned window alone; a tight buffer and
    a wider padded buffer (an all-gather slot) hold the same bits."""
    from svi_hip import _lib as L
    v, _ = vae
    _, seed, shape, split = CASES[3]
    vid, want = whole_encode(v, seed, shape)
    hh, ww, tl = shape[2] // 8, shape[3] // 8, want.shape[1]
    for p in range(4):
        h0, h1, w0, w1 = L.vae_encode_split_plan(hh, ww, *split, p)["owned"]
        full = torch.full((tl, hh, ww, 384), 7.5e8, device="cuda")
        assert v.encode_part(vid, split, p, out=full) is full
        inside = torch.zeros((hh, ww), dtype=torch.bool, device="cuda")
        inside[h0:h1, w0:w1] = True
        assert bool((full[:, ~inside] == 7.5e8).all())
        assert bool((full[:, inside] != 7.5e8).all()) and torch.isfinite(full).all()
        tight = v.encode_part(vid, split, p)
        assert tuple(tight.shape) == (tl, h1 - h0, w1 - w0, 384)
        assert torch.equal(tight, full[:, h0:h1, w0:w1])
        padded = torch.full((tl, h1 - h0 + 3, w1 - w0 + 5, 384), 7.5e8, device="cuda")
        v.encode_part(vid, split, p, out=padded)
        assert torch.equal(padded[:, :h1 - h0, :w1 - w0], tight)
        assert bool((padded[:, h1 - h0:] == 7.5e8).all()) and bool((padded[:, :, w1 - w0:] == 7.5e8).all())


def test_one_part_is_todays_encode(vae):
    v, _ = vae
    vid, want = whole_encode(v, 713, (3, 5, 40, 56))
    assert torch.equal(v.encode([vid], device="cuda", split=(1, 1))[0], want)
    assert torch.equal(v.encode_tail(v.encode_part(vid, (1, 1), 0)), want)


def test_one_part_at_other_pitches_is_the_whole_front(vae):
    """One part into a feature buffer 3 rows and 5 columns larger than the map: the window holds the bits of part 0 written into a tight
    buffer, nothing outside it is written, and the tail of the tight buffer is the whole encode bit for bit (the part form of the encoder
    front with a trivial plan is the whole front)."""
    v, _ = vae
    vid, want = whole_encode(v, 713, (3, 5, 40, 56))
    tl, hh, ww = want.shape[1], 40 // 8, 56 // 8
    tight = v.encode_part(vid, (1, 1), 0)
    assert tuple(tight.shape) == (tl, hh, ww, 384)
    padded = torch.full((tl, hh + 3, ww + 5, 384), 7.5, device="cuda")
    assert v.encode_part(vid, (1, 1), 0, out=padded) is padded
    assert torch.equal(padded[:, :hh, :ww], tight)
    assert bool((padded[:, hh:] == 7.5).all()) and bool((padded[:, :, ww:] == 7.5).all())
    assert torch.equal(v.encode_tail(tight), want)


def test_refusals(vae):
    v, _ = vae
    vid, _ = whole_encode(v, 713, (3, 5, 40, 56))
    with pytest.raises(ValueError, match="tiled"):
        v.encode([vid], device="cuda", tiled=True, split=(1, 2))
    with pytest.raises(RuntimeError, match="without a pixel"):
        v.encode([vid], device="cuda", split=(1, 8))
    with pytest.raises(RuntimeError, match="outside"):
        v.encode_part(vid, (1, 2), 2)
    with pytest.raises(ValueError, match="group needs split"):
        v.encode([vid], device="cuda", group=object())


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
        vid = torch.from_numpy(np.tanh(synth.randn(714, 3, 5, 128, 256))).cuda()
        whole = v.encode([vid], device="cuda")[0]
        refused = False
        try:
            v.encode([vid], device="cuda", split=(2, 2), group=dist.group.WORLD)       # four parts, two ranks: refused before any collective
        except ValueError as ex:
            refused = "needs a group of 4 ranks" in str(ex)
        got = v.encode([vid], device="cuda", split=(1, 2), group=dist.group.WORLD)[0]
        r, mx, _ = errs(got, whole)
        gathered = [torch.empty(got.shape, dtype=torch.float32) for _ in range(world)]
        dist.all_gather(gathered, got.cpu())
        same = all(torch.equal(g, gathered[0]) for g in gathered)
        queue.put((rank, r, mx, bool(refused), bool(same)))
    finally:
        dist.destroy_process_group()


def test_two_ranks_over_gloo():
    """Two gloo ranks on the one GPU, fresh child processes: encode(split=(1, 2), group=world) on (3, 5, 128, 256) — each rank encodes its half
    into its slot, one all-gather assembles the feature map and both run the tail; a group whose size does not match the split is refused
    before any collective."""
    from spawn_util import run_ranks
    res = run_ranks(_two_rank_worker, 2, timeout=300)
    report("vae_encode_split_two_ranks", ranks=[list(r) for r in sorted(res)])
    print(sorted(res))
    assert sorted(r[0] for r in res) == [0, 1], res
    assert all(r[3] for r in res), res                           # the 2 x 2 split on two ranks was refused
    assert all(r[4] for r in res), res                           # the same latents on both ranks, bit for bit
    assert all(r[1] < REL and r[2] < MAXABS for r in res), res


def test_stream_loop_with_a_split_encode():
    """StreamLoop, tiny I2V synth model, 2 clips of 2 steps at 32 x 48.  vae_encode_split=(1, 2) in local mode: 8-bit frames within 1 code value
    of the plain stream's.  A stream that only sets vae_split is what it was: bit-equal to the same stream with vae_encode_split=None spelled out."""
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
    loop = svi_hip.StreamLoop(dit, v, vae_encode_split=(1, 2), **kw)
    assert loop.vae_encode_split == dict(split=(1, 2), group=None) and loop.vae_split == {}
    split = loop.run(img, ref, prompts, CLIPS)
    assert split.dtype == torch.uint8 and split.shape == plain.shape
    diff = (split.int() - plain.int()).abs()
    n = int((diff > 0).sum())
    report("vae_encode_split_stream", pixels=int(diff.numel()), differing=n, max_code_diff=int(diff.max()))
    print(f"stream: {n} of {diff.numel()} 8-bit values differ, max {int(diff.max())}")
    assert int(diff.max()) <= 1
    only_decode = svi_hip.StreamLoop(dit, v, vae_split=(1, 2), **kw)
    assert only_decode.vae_encode_split == {}
    a = only_decode.run(img, ref, prompts, CLIPS)
    b = svi_hip.StreamLoop(dit, v, vae_split=(1, 2), vae_encode_split=None, **kw).run(img, ref, prompts, CLIPS)
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match="process group"):
        svi_hip.StreamLoop(dit, v, vae_encode_split=True, **kw)
