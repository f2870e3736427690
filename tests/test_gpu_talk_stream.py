"""-m gpu: the resident clip loop of a talk stream (svi_hip.TalkStreamLoop; test_svi_talk.py:277-302 around SVITalkVideoPipeline.__call__).

Every stage is pinned elsewhere against the reference — the talk sampler (golden/dit_tiny_talk.npz), the VAE, encode_images_adaptive, the 8-bit
hand-off.  Here: the stream — one resident loop, the audio windows cut and the slots re-staged on the device at every clip boundary, every clip after
the first a replay — gives, frame for frame in uint8, what a loop written out by hand gives: per clip one DenoiseLoop(graph=False).sample_multitalk call
(three eager forwards per step) on windows built on the host, with the VAE calls and the 8-bit hand-off by hand.  Same kernels on the same values, so the
comparison is torch.equal."""
import pytest
import torch

import synth
from audio_window_cases import host_tuples, window_rows
from gpu_util import dev

pytestmark = pytest.mark.gpu

CFG = synth.TINY_DIT_TALK
H, W, NF, STEPS, CLIPS, TLAT = 32, 48, 9, 2, 3, 3
N_AUDIO = 20                  # the audio ends inside clip 2 (frames 17 .. 25 with one motion frame, 13 .. 21 with five)
SCALES = dict(audio=4.0, text=5.0)
TEA_MODEL = "Wan2.1-I2V-14B-720P"
_SHARED = {}


def _shared():
    """Two DiTs of the same weights (the eager loops toggle their model's context cache: they get a model of their own), the VAE and the stream's inputs."""
    import svi_hip
    if not _SHARED:
        sd = {k: torch.from_numpy(v) for k, v in synth.dit_state_dict(synth.TALK_SEED, **CFG).items()}
        mk = lambda: svi_hip.WanDiT.from_state_dict(sd, eps=1e-6, num_heads=synth.num_heads_of(CFG), **CFG)      # noqa: E731
        _SHARED.update(dit=mk(), ref=mk(), vae=svi_hip.WanVideoVAE.from_state_dict({k: torch.from_numpy(v) for k, v in synth.vae_state_dict(500).items()}),
                       img=torch.from_numpy(synth.condition_frames(31, 1, H, W)), ref_frame=torch.from_numpy(synth.condition_frames(32, 1, H, W)[0]),
                       prompt=(dev(synth.text_context(40, 16, CFG["text_dim"], 9)), dev(synth.text_context(50, 16, CFG["text_dim"], 5))),
                       clipf=dev(synth.randn(33, 1, 257, 1280)), emb=torch.from_numpy(0.5 * synth.randn(34, N_AUDIO, 12, 768)))
    return _SHARED


def _by_hand(s, n_motion, seeds, steps, tea):
    """The reference's outer loop, written out: cursor, host-built windows, one eager sampler call per clip, decode, 8 bit, hand-off, whole clips stitched."""
    import svi_hip
    motion = s["img"].cuda()
    refv = svi_hip.u8_to_video(s["ref_frame"][None].cuda())[0]
    clips = []
    for k in range(CLIPS):
        start = k * NF - (n_motion if k > 0 else 0)
        aud, null = host_tuples(s["emb"], start, TLAT)
        y = svi_hip.image_condition(s["vae"], svi_hip.u8_to_video(motion), refv, NF, False, -1)
        lat = svi_hip.generate_noise((1, 16, TLAT, H // 8, W // 8), seed=seeds[k], device="cpu", dtype=torch.float32).to("cuda", torch.bfloat16)
        lat = svi_hip.DenoiseLoop(s["ref"], graph=False).sample_multitalk(lat, *s["prompt"], aud, null, num_inference_steps=steps, text_scale=SCALES["text"],
                                                                          audio_scale=SCALES["audio"], y=y, clip_feature=s["clipf"], **tea)
        frames = svi_hip.video_to_u8(s["vae"].decode(lat.float(), device="cuda")[0])
        clips.append(dict(start=start, latents=lat, frames=frames))
        motion = frames[-n_motion:]
    return clips


# the issue's cases: 2 steps, 1 and 5 motion frames, TeaCache off and on; with 2 steps TeaCache never skips (the first and the last step compute), so one
# more case runs 4 steps under a threshold no drift reaches: the middle steps skip, on graphs of their own mode triples (four of them: what the loop holds)
@pytest.mark.parametrize("n_motion,steps,thresh", [(1, 2, None), (5, 2, None), (1, 2, 0.3), (5, 2, 0.3), (1, 4, 1e9)],
                         ids=["m1", "m5", "m1-tea", "m5-tea", "m1-tea-skips"])
def test_talk_stream_is_the_hand_written_clip_loop(n_motion, steps, thresh):
    import svi_hip
    s = _shared()
    tea = {} if thresh is None else dict(tea_cache_l1_thresh=thresh, tea_cache_model_id=TEA_MODEL)
    seeds = [5, 5, 5] if n_motion == 1 else [3, 45, 87]                      # the reference's call: one seed for the stream; or one per clip
    sl = svi_hip.TalkStreamLoop(s["dit"], s["vae"], clip_encoder=lambda first: s["clipf"], num_motion_frames=n_motion, num_frames=NF,
                                num_inference_steps=steps, cfg_scale=SCALES, ref_pad_num=-1, **tea)
    assert sl.loop.graph and sl.loop.resident
    gen_before = s["dit"].generation()
    video = sl.run(s["img"], s["ref_frame"], s["prompt"], s["emb"], CLIPS, seed=seeds[0] if n_motion == 1 else seeds)
    tr = sl.trace
    assert video.dtype == torch.uint8 and tuple(video.shape) == (CLIPS * NF, H, W, 3)                  # every clip whole
    assert not s["dit"]._ctx_cache_on and not s["dit"]._audio_slots                                      # the model comes back as it was handed in
    assert [t["audio_start"] for t in tr] == [0, NF - n_motion, 2 * NF - n_motion] and [t["seed"] for t in tr] == seeds
    want = _by_hand(s, n_motion, seeds, steps, tea)
    for k in range(CLIPS):
        assert tr[k]["audio_start"] == want[k]["start"]
        if k:
            assert torch.equal(tr[k]["motion"], tr[k - 1]["frames"][-n_motion:])
        assert torch.equal(tr[k]["latents"], want[k]["latents"]), k
        assert torch.equal(tr[k]["frames"], want[k]["frames"]), k
    assert torch.equal(video, torch.cat([c["frames"] for c in want]))
    # one resident loop: what was captured for clip 0 is what clips 1 and 2 replayed — the same count and the very same graph objects
    assert tr[0]["captures"] >= 1 and tr[2]["captures"] == tr[0]["captures"], [t["captures"] for t in tr]
    held = {id(g) for g in tr[0]["graphs"]}                   # (trace keeps the graph objects alive: an id is not reused)
    assert len(held) >= 1 and all({id(g) for g in t["graphs"]} == held for t in tr)
    if thresh is None:
        assert tr[0]["captures"] == 1
    if steps == 4:
        assert sl.loop.tea_counts["skipped"] >= 1 and tr[0]["captures"] >= 2
    # the clip boundaries moved nothing a captured graph relies on
    assert tr[0]["generation"] != gen_before and tr[1]["generation"] == tr[0]["generation"] and tr[2]["generation"] == tr[0]["generation"]
    # the audio ended inside clip 2: its late windows all read the last row, and the clip was produced all the same
    first, latter = window_rows(N_AUDIO, TLAT, tr[2]["audio_start"])
    assert int(first.min()) < N_AUDIO - 1 and latter[-1].tolist()[-3:] == [N_AUDIO - 1] * 3 and 2 * NF - n_motion + NF > N_AUDIO
    assert tr[2]["frames"].float().std() > 0


def test_a_talk_stream_that_fails_midway_hands_the_model_back():
    """The clip encoder raises at clip 1, behind clip 0's capture, staged audio slots and context cache: run() passes the error on and leaves none of
    them; the same loop object then runs the stream as a newly built one does."""
    import svi_hip
    s, calls = _shared(), []

    def encoder(first):
        calls.append(first)
        if len(calls) == 2:
            raise RuntimeError("the clip encoder failed")
        return s["clipf"]
    mk = lambda enc: svi_hip.TalkStreamLoop(s["dit"], s["vae"], clip_encoder=enc, num_motion_frames=1, num_frames=NF, num_inference_steps=STEPS,      # noqa: E731
                                            cfg_scale=SCALES, ref_pad_num=-1)
    sl = mk(encoder)
    with pytest.raises(RuntimeError, match="the clip encoder failed"):
        sl.run(s["img"], s["ref_frame"], s["prompt"], s["emb"], 2, seed=5)
    assert len(calls) == 2 and len(sl.trace) == 1 and sl.trace[0]["captures"] == 1                      # clip 0 ran, on a captured step
    assert s["dit"]._ctx_cache_on is False and not s["dit"]._audio_slots and sl.loop.held_graphs() == []
    again = sl.run(s["img"], s["ref_frame"], s["prompt"], s["emb"], 2, seed=5)
    fresh = mk(lambda first: s["clipf"]).run(s["img"], s["ref_frame"], s["prompt"], s["emb"], 2, seed=5)
    assert len(calls) == 4 and tuple(again.shape) == (2 * NF, H, W, 3) and torch.equal(again, fresh)
    assert s["dit"]._ctx_cache_on is False and not s["dit"]._audio_slots


def test_talk_stream_refusals():
    import svi_hip
    s = _shared()
    with pytest.raises(ValueError, match="CFG-pair"):
        svi_hip.TalkStreamLoop(s["dit"], s["vae"], cfg_pair=object())
    with pytest.raises(ValueError, match="4 k \\+ 1"):
        svi_hip.TalkStreamLoop(s["dit"], s["vae"], num_frames=10)
    with pytest.raises(ValueError, match="dict\\(audio=, text=\\)"):
        svi_hip.TalkStreamLoop(s["dit"], s["vae"], cfg_scale=dict(text=5.0))
    sl = svi_hip.TalkStreamLoop(s["dit"], s["vae"], num_frames=NF, num_inference_steps=STEPS)
    with pytest.raises(ValueError, match="12, 768"):
        sl.run(s["img"], s["ref_frame"], s["prompt"], s["emb"][:, :6], 1, clip_feature=s["clipf"])
    with pytest.raises(ValueError, match="seeds"):
        sl.run(s["img"], s["ref_frame"], s["prompt"], s["emb"], 2, seed=[1], clip_feature=s["clipf"])
    loop = svi_hip.DenoiseLoop(s["dit"], graph=True)
    lat = torch.zeros((1, 16, TLAT, H // 8, W // 8), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError, match="not staged"):
        loop.sample_multitalk(lat, *s["prompt"], None, None, num_inference_steps=2, clip_feature=s["clipf"], y=torch.zeros((1, 20, TLAT, H // 8, W // 8), device="cuda"))
    with pytest.raises(ValueError, match="eager forwards need"):
        svi_hip.DenoiseLoop(s["dit"], graph=False).sample_multitalk(lat, *s["prompt"], None, None, num_inference_steps=2)


def test_example_launcher_runs_a_synthetic_talk_stream(tmp_path):
    """examples/test_svi_talk_hip.py --synthetic: the reference CLI's surface over the whole chain on a box with no weights and no audio encoder: 3 clips
    of 9 frames, every clip whole, the cursor 0 / 8 / 17, one captured step graph; the script does not import wav2vec2."""
    import json
    import os
    import subprocess
    import sys
    import numpy as np
    from conftest import ROOT
    script = os.path.join(ROOT, "examples", "test_svi_talk_hip.py")
    assert "import transformers" not in open(script).read() and "Wav2Vec2" not in open(script).read()
    r = subprocess.run([sys.executable, script, "--synthetic", "--num_clips", "3", "--num_steps", "3", "--height", "32", "--width", "48", "--max_frames", "9",
                        "--output", str(tmp_path), "--ref_pad_num", "-1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    rec = json.loads([l for l in r.stdout.splitlines() if l.startswith('{"test_svi_talk_hip"')][-1])["test_svi_talk_hip"][0]
    assert rec["clips"] == 3 and rec["frames"] == 27 and rec["audio_starts"] == [0, 8, 17] and rec["step_graph_captures"] == 1
    assert rec["audio_frames"] < 17 + 9                        # the stream outlasts its audio
    vid = np.load(os.path.join(rec["out"], "video_u8.npy"))
    assert vid.shape == (27, 32, 48, 3) and vid.dtype == np.uint8 and vid.std() > 0
