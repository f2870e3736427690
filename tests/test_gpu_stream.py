"""-m gpu: the resident clip loop of an image-conditioned stream (svi_hip.StreamLoop, test_svi.py:424-476 around __call__).
Every stage is pinned elsewhere (DiT, scheduler, VAE, encode_images_adaptive); here: the 8-bit frame hand-off is the reference's
host arithmetic bit for bit, and the loop composes the stages as the reference's loop does (seeds, prompt cycling, motion frames =
the last 8-bit frames of the previous clip, stitching rule)."""
import numpy as np
import pytest
import torch

import synth
from gpu_util import dev

pytestmark = pytest.mark.gpu


def test_u8_round_trip_matches_host_arithmetic():
    import svi_hip
    rs = np.random.RandomState(3)
    v = rs.uniform(-1.3, 1.3, size=(3, 4, 10, 14)).astype(np.float32)
    v.flat[:8] = [-1.0, 1.0, 0.0, -0.99607843, 0.00392157, 1.0000001, -1.0000001, 0.5]      # edges, exact grid points
    want = ((np.transpose(v, (1, 2, 3, 0)) + 1) * 127.5).clip(0, 255).astype(np.uint8)       # tensor2video, svi_video.py:367-368
    got = svi_hip.video_to_u8(torch.from_numpy(v).cuda())
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    frames = rs.randint(0, 256, size=(5, 10, 14, 3)).astype(np.uint8)
    want_f = synth.frames_to_tensor(frames)                                                   # preprocess_image, base.py:44-45
    got_f = svi_hip.u8_to_video(torch.from_numpy(frames).cuda())
    assert np.array_equal(got_f.cpu().numpy(), want_f)
    # note: with the reference's truncating cast quantise(dequantise(x)) is NOT the identity (201 -> 200.99998 -> 200); the
    # device kernels reproduce exactly that, they do not "fix" it
    back = svi_hip.video_to_u8(got_f.permute(1, 0, 2, 3).contiguous()).cpu().numpy()
    host = ((np.transpose(want_f, (0, 2, 3, 1)) + 1) * 127.5).clip(0, 255).astype(np.uint8)
    assert np.array_equal(back, host)


@pytest.mark.parametrize("n_motion", [1, 2])
def test_stream_loop_composition(n_motion):
    import svi_hip
    c = synth.TINY_DIT_I2V
    sd = {k: torch.from_numpy(v) for k, v in synth.dit_state_dict(200, **c).items()}
    dit = svi_hip.WanDiT.from_state_dict(sd, eps=1e-6, num_heads=synth.num_heads_of(c), **c)
    vae = svi_hip.WanVideoVAE.from_state_dict({k: torch.from_numpy(v) for k, v in synth.vae_state_dict(500).items()})
    H, W, NF, STEPS, CLIPS = 32, 48, 9, 2, 3
    img = torch.from_numpy(synth.condition_frames(31, 1, H, W))
    ref = torch.from_numpy(synth.condition_frames(32, 1, H, W)[0])
    prompts = [(dev(synth.text_context(40 + i, 16, c["text_dim"], 9)), dev(synth.text_context(50 + i, 16, c["text_dim"], 5))) for i in range(2)]
    clipf = dev(synth.randn(33, 1, 257, 1280))
    sl = svi_hip.StreamLoop(dit, vae, clip_encoder=lambda first: clipf, num_motion_frames=n_motion, num_frames=NF,
                            num_inference_steps=STEPS, ref_pad_num=-1)
    video = sl.run(img, ref, prompts, CLIPS)
    assert video.dtype == torch.uint8 and tuple(video.shape) == ((NF - n_motion) * (CLIPS - 1) + NF, H, W, 3)
    tr = sl.trace
    assert sl.loop.resident and sl.loop.captures == 1                                        # three clips, ONE captured step graph (replayed by clips 2 and 3)
    assert not dit._ctx_cache_on                                                             # the model comes back as it was handed in
    assert [t["seed"] for t in tr] == [0, 42, 84]                                            # seed = chunk_idx * seed_times
    assert torch.equal(tr[0]["motion"].cpu(), img)
    refv = svi_hip.u8_to_video(ref[None].cuda())[0]
    for k in range(CLIPS):
        if k:
            assert torch.equal(tr[k]["motion"], tr[k - 1]["frames"][-n_motion:])             # hand-off: the previous clip's last 8-bit frames
        y = svi_hip.image_condition(vae, svi_hip.u8_to_video(tr[k]["motion"]), refv, NF, False, -1)
        assert torch.equal(y, tr[k]["y"])
        # the clip itself: the plain denoise loop on (seed_k, prompt_k, y_k), then decode -> 8 bit
        lat = svi_hip.generate_noise((1, 16, 3, H // 8, W // 8), seed=42 * k, device="cpu", dtype=torch.float32).to("cuda", torch.bfloat16)
        cp, cn = prompts[k % 2]
        lat = svi_hip.DenoiseLoop(dit).sample(lat, cp, cn, num_inference_steps=STEPS, y=y, clip_feature=clipf)
        assert torch.equal(lat, tr[k]["latents"])
        assert torch.equal(svi_hip.video_to_u8(vae.decode(lat.float(), device="cuda")[0]), tr[k]["frames"])
    stitched = torch.cat([t["frames"][:-n_motion] for t in tr[:-1]] + [tr[-1]["frames"]])
    assert torch.equal(video, stitched)


def test_a_stream_that_fails_midway_hands_the_model_back():
    """The clip encoder raises at clip 1, behind clip 0's capture and context cache: run() passes the error on and leaves neither; the same loop object
    then runs the stream as a newly built one does."""
    import svi_hip
    c = synth.TINY_DIT_I2V
    sd = {k: torch.from_numpy(v) for k, v in synth.dit_state_dict(200, **c).items()}
    dit = svi_hip.WanDiT.from_state_dict(sd, eps=1e-6, num_heads=synth.num_heads_of(c), **c)
    vae = svi_hip.WanVideoVAE.from_state_dict({k: torch.from_numpy(v) for k, v in synth.vae_state_dict(500).items()})
    H, W, NF, STEPS, CLIPS = 32, 48, 9, 2, 2
    img = torch.from_numpy(synth.condition_frames(31, 1, H, W))
    ref = torch.from_numpy(synth.condition_frames(32, 1, H, W)[0])
    prompts = [(dev(synth.text_context(40 + i, 16, c["text_dim"], 9)), dev(synth.text_context(50 + i, 16, c["text_dim"], 5))) for i in range(2)]
    clipf, calls = dev(synth.randn(33, 1, 257, 1280)), []

    def encoder(first):
        calls.append(first)
        if len(calls) == 2:
            raise RuntimeError("the clip encoder failed")
        return clipf
    mk = lambda enc: svi_hip.StreamLoop(dit, vae, clip_encoder=enc, num_motion_frames=1, num_frames=NF, num_inference_steps=STEPS, ref_pad_num=-1)      # noqa: E731
    sl = mk(encoder)
    with pytest.raises(RuntimeError, match="the clip encoder failed"):
        sl.run(img, ref, prompts, CLIPS)
    assert len(calls) == 2 and len(sl.trace) == 1 and sl.loop.captures == 1                             # clip 0 ran, on a captured step
    assert dit._ctx_cache_on is False and not dit._audio_slots and sl.loop.held_graphs() == []
    again = sl.run(img, ref, prompts, CLIPS)
    fresh = mk(lambda first: clipf).run(img, ref, prompts, CLIPS)
    assert len(calls) == 4 and tuple(again.shape) == (NF - 1 + NF, H, W, 3) and torch.equal(again, fresh)
    assert dit._ctx_cache_on is False


@pytest.mark.parametrize("case", synth.STREAM_CASES, ids=lambda c: c["name"])
def test_stream_against_the_reference_clip_loop(case, golden):
    """Rows a23 / b against the reference itself: golden/clip_stream.npz holds what the reference's own clip loop (test_svi.py:424-485)
    around its own SVIVideoPipeline.__call__ (svi_video.py:423-520) produced on a tiny I2V stream (gen_golden.py::gen_clip_stream).
      * tensor2video on the reference's float video: bit-identical 8-bit frames;
      * schedule: seeds, prompt cycling, which (clip, frame) every stitched frame is;
      * values: every clip re-run from the reference's own hand-off frames (teacher-forced), and the free-running stream.
    The reference ran its DiT in bf16 on the CPU; two bf16 implementations differ in rounding order, so 8-bit frames agree to within a
    level or two, not bit for bit: mean |diff| <= 0.75 level teacher-forced and free-running, no pixel off by more than 6
    (measured: mean 0.41-0.44 levels, max 3, 59-60 % of all pixels identical; profiles/r2a_parity_report.jsonl)."""
    import svi_hip
    from svi_hip.parallel import clip_prompt_index, clip_seed
    g, name = golden("clip_stream.npz"), case["name"]
    ref_frames, stitched_ref = g[name + "_frames"], g[name + "_stitched"]
    got0 = svi_hip.video_to_u8(torch.from_numpy(g[name + "_video_f32_clip0"]).cuda()).cpu().numpy()
    assert np.array_equal(got0, ref_frames[0])
    c = synth.TINY_DIT_I2V
    sd = {k: torch.from_numpy(v) for k, v in synth.dit_state_dict(200, **c).items()}
    dit = svi_hip.WanDiT.from_state_dict(sd, eps=1e-6, num_heads=synth.num_heads_of(c), **c)
    vae = svi_hip.WanVideoVAE.from_state_dict({k: torch.from_numpy(v) for k, v in synth.vae_state_dict(500).items()})
    H, W = synth.STREAM_HW
    n_motion, NF, CLIPS = case["num_motion_frames"], case["num_frames"], case["num_clips"]
    img = torch.from_numpy(synth.condition_frames(synth.STREAM_IMAGE_SEED, 1, H, W))
    neg = dev(synth.text_context(synth.STREAM_PROMPT_SEED + 50, 16, c["text_dim"], 5))
    prompts = [(dev(synth.text_context(synth.STREAM_PROMPT_SEED + i, 16, c["text_dim"], 9)), neg) for i in range(case["num_prompts"])]
    clipf = dev(synth.randn(synth.STREAM_CLIP_SEED, 1, 257, 1280))
    sl = svi_hip.StreamLoop(dit, vae, clip_encoder=lambda first: clipf, num_motion_frames=n_motion, num_frames=NF,
                            num_inference_steps=case["steps"], ref_pad_cfg=case["ref_pad_cfg"], ref_pad_num=case["ref_pad_num"])
    kw = dict(prompt_repeat_times=case["prompt_repeat_times"], use_first_prompt_only=case["use_first_prompt_only"])
    # ---- schedule
    assert [clip_seed(k) for k in range(CLIPS)] == [int(s) for s in g[name + "_seeds"]]
    assert [clip_prompt_index(k, len(prompts), case["prompt_repeat_times"], case["use_first_prompt_only"]) for k in range(CLIPS)] == \
        [int(p) for p in g[name + "_prompts"]]
    assert np.array_equal(g[name + "_motion0"], img.numpy())
    for k in range(1, CLIPS):                                   # the reference hands over the last frames of the previous clip
        assert np.array_equal(g[f"{name}_motion{k}"], ref_frames[k - 1][-n_motion:])
    where = []                                                  # stitched frame i = frame j of clip k in the reference's video
    for k in range(CLIPS):
        keep = NF if k == CLIPS - 1 else NF - n_motion
        where += [(k, j) for j in range(keep)]
    assert len(where) == len(stitched_ref) and all(np.array_equal(stitched_ref[i], ref_frames[k][j]) for i, (k, j) in enumerate(where))
    # ---- values, teacher-forced: clip k from the reference's own hand-off frames
    worst_mean, worst_max = 0.0, 0
    for k in range(CLIPS):
        motion = torch.from_numpy(g[f"{name}_motion{k}"])
        out = sl.run(motion, img[0], prompts, k + 1, start_clip=k, **kw).cpu().numpy().astype(np.int32)
        assert [t["seed"] for t in sl.trace] == [42 * k]
        d = np.abs(out - ref_frames[k].astype(np.int32))
        worst_mean, worst_max = max(worst_mean, float(d.mean())), max(worst_max, int(d.max()))
    # ---- the free-running stream
    video = sl.run(img, img[0], prompts, CLIPS, **kw)
    tr = sl.trace
    assert tuple(video.shape) == stitched_ref.shape
    assert all(torch.equal(video[i], tr[k]["frames"][j]) for i, (k, j) in enumerate(where))
    d = np.abs(video.cpu().numpy().astype(np.int32) - stitched_ref.astype(np.int32))
    from gpu_util import report
    report("clip_stream", case=name, forced_mean_levels=worst_mean, forced_max_levels=worst_max, stream_mean_levels=float(d.mean()),
           stream_max_levels=int(d.max()), stream_frac_equal=float((d == 0).mean()))
    assert worst_mean <= 0.75 and worst_max <= 6, (worst_mean, worst_max)
    assert float(d.mean()) <= 0.75 and int(d.max()) <= 6, (float(d.mean()), int(d.max()))


def test_example_launcher_runs_a_synthetic_window(tmp_path):
    """examples/test_svi_hip.py --synthetic: the reference CLI's surface over the whole HIP chain — random-init I2V model, seeded prompt embeddings, a
    synthetic image, StreamLoop (conditioning encode, CFG denoise on one captured step graph, decode, 8-bit hand-off, stitching) — on a box
    with no weights: 3 clips of 9 frames, motion hand-off of 1 frame -> 8 + 8 + 9 stitched frames, seeds 0 / 42 / 84, one graph capture."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "test_svi_hip.py"), "--synthetic", "--synthetic_model", "tiny-i2v", "--num_clips", "3",
                        "--num_steps", "3", "--height", "32", "--width", "48", "--max_frames", "9", "--output", str(tmp_path), "--ref_pad_num", "-1"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    rec = json.loads([l for l in r.stdout.splitlines() if l.startswith('{"test_svi_hip"')][-1])["test_svi_hip"][0]
    assert rec["clips"] == 3 and rec["frames"] == 8 + 8 + 9 and rec["seeds"] == [0, 42, 84] and rec["step_graph_captures"] == 1
    vid = np.load(os.path.join(rec["out"], "video_u8.npy"))
    assert vid.shape == (25, 32, 48, 3) and vid.dtype == np.uint8 and vid.std() > 0
