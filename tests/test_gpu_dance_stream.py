"""-m gpu: the resident clip loop of a dance stream (svi_hip.DanceStreamLoop; test_svi_dance.py:238-288 around SVIDanceVideoPipeline.__call__).

Every stage is pinned elsewhere against the reference — the pose embedder (golden/pose_embed.npz), the sampler's branch rule (golden/dance_sampler.npz),
the pose windows (golden/dance_stream.npz), the VAE, encode_images_adaptive, the 8-bit hand-off.  Here: the stream — one resident loop, the pose window
cut on the device at every clip boundary, every clip after the first a replay — gives, bit for bit in frames, latents and y of every clip, what a loop
written out by hand gives: per clip the window built on the host (tests/dance_stream_cases.py, held to the fixture on the CPU) and uploaded,
PoseEmbedder.__call__, one non-resident DenoiseLoop(graph=False).sample call, decode, 8 bit, hand-off.  Same kernels on the same values, so the
comparison is torch.equal."""
import pytest
import torch

import synth
from dance_stream_cases import CASES, frame_table, host_window, pose_source
from gpu_util import dev

pytestmark = pytest.mark.gpu

CFG = synth.TINY_DIT_I2V
H, W, NF, CLIPS, TLAT = 32, 48, 9, 3, 3
SCALES = dict(audio=1.0, text=2.0)          # the script's defaults
TEA_MODEL = "Wan2.1-I2V-14B-720P"
_SHARED = {}


def _shared():
    """Two DiTs of the same weights (the eager loops toggle their model's context cache: they get a model of their own), the pose embedder of their
    width, the VAE and the stream's inputs.  Pose videos: 23 frames of 20 x 27 (padded columns; wraps in clip 2), and 7 frames of 9 x 11, shorter than a clip."""
    import svi_hip
    if not _SHARED:
        sd = {k: torch.from_numpy(v) for k, v in synth.dit_state_dict(200, **CFG).items()}
        mk = lambda: svi_hip.WanDiT.from_state_dict(sd, eps=1e-6, num_heads=synth.num_heads_of(CFG), **CFG)      # noqa: E731
        pose_sd = {k: torch.from_numpy(v) for k, v in synth.pose_state_dict(synth.POSE_SEED, dim=CFG["dim"]).items()}
        _SHARED.update(dit=mk(), ref=mk(), pose=svi_hip.PoseEmbedder.from_state_dict(pose_sd),
                       vae=svi_hip.WanVideoVAE.from_state_dict({k: torch.from_numpy(v) for k, v in synth.vae_state_dict(500).items()}),
                       img=torch.from_numpy(synth.condition_frames(31, 1, H, W)), ref_frame=torch.from_numpy(synth.condition_frames(32, 1, H, W)[0]),
                       prompt=(dev(synth.text_context(40, 16, CFG["text_dim"], 9)), dev(synth.text_context(50, 16, CFG["text_dim"], 5))),
                       clipf=dev(synth.randn(33, 1, 257, 1280)), long=pose_source("pad_w"), short=pose_source("upscale_short"))
        assert tuple(CASES["pad_w"][3:6]) == (H, W, NF) and tuple(CASES["upscale_short"][3:6]) == (H, W, NF)
    return _SHARED


def _by_hand(s, pose, n_motion, seeds, steps, wo, remove, tea):
    """The reference's outer loop, written out: the pose window built on the host and uploaded, the embedder, one eager sampler call per clip, decode,
    8 bit, hand-off."""
    import svi_hip
    motion = s["img"].cuda()
    refv = svi_hip.u8_to_video(s["ref_frame"][None].cuda())[0]
    clips = []
    for k in range(CLIPS):
        y = svi_hip.image_condition(s["vae"], svi_hip.u8_to_video(motion), refv, NF, False, -1)
        cond = dict(y=y, clip_feature=s["clipf"])
        if not remove:
            cond["add_condition"] = s["pose"](host_window(pose, k, NF, n_motion, H, W).cuda())
        lat = svi_hip.generate_noise((1, 16, TLAT, H // 8, W // 8), seed=seeds[k], device="cpu", dtype=torch.float32).to("cuda", torch.bfloat16)
        lat = svi_hip.DenoiseLoop(s["ref"], graph=False).sample(lat, *s["prompt"], num_inference_steps=steps, cfg_scale=SCALES["text"], cond_wo_pose=wo,
                                                                **tea, **cond)
        frames = svi_hip.video_to_u8(s["vae"].decode(lat.float(), device="cuda")[0])
        clips.append(dict(y=y, latents=lat, frames=frames, add_condition=cond.get("add_condition")))
        motion = frames[-n_motion:]
    return clips


# (motion frames, pose video, cond_wo_pose, remove_pose, steps, TeaCache threshold).  With 2 steps TeaCache never skips (the first and the last step
# compute), so the TeaCache cases run 4 steps: at 0.3 the caches decide by the drift, at 1e9 every step that may skip does.
@pytest.mark.parametrize("n_motion,video,wo,remove,steps,thresh",
                         [(1, "long", True, False, 2, None), (5, "long", True, False, 2, None), (1, "long", False, False, 2, None),
                          (5, "short", False, False, 2, None), (1, "short", True, False, 2, None), (1, "long", True, True, 2, None),
                          (1, "long", True, False, 4, 0.3), (5, "short", False, False, 4, 1e9)],
                         ids=["m1", "m5", "m1-cond-only", "m5-short-cond-only", "m1-short", "m1-remove-pose", "m1-tea", "m5-short-cond-only-tea-skips"])
def test_dance_stream_is_the_hand_written_clip_loop(n_motion, video, wo, remove, steps, thresh):
    import svi_hip
    s = _shared()
    pose = s[video]
    tea = {} if thresh is None else dict(tea_cache_l1_thresh=thresh, tea_cache_model_id=TEA_MODEL)
    seeds = [5, 5, 5] if n_motion == 1 else [3, 45, 87]                      # one seed for the stream, or one per clip
    sl = svi_hip.DanceStreamLoop(s["dit"], s["vae"], s["pose"], clip_encoder=lambda first: s["clipf"], num_motion_frames=n_motion, num_frames=NF,
                                 num_inference_steps=steps, cfg_scale=SCALES, cond_wo_pose=wo, remove_pose=remove, ref_pad_num=-1, **tea)
    assert sl.loop.graph and sl.loop.resident
    video_u8 = sl.run(s["img"], s["ref_frame"], s["prompt"], pose, CLIPS, seed=seeds[0] if n_motion == 1 else seeds)
    tr = sl.trace
    assert video_u8.dtype == torch.uint8 and tuple(video_u8.shape) == ((NF - n_motion) * (CLIPS - 1) + NF, H, W, 3)
    assert not s["dit"]._ctx_cache_on                                        # the model comes back as it was handed in
    assert [t["pose_window"] for t in tr] == ([None] * CLIPS if remove else list(range(CLIPS))) and [t["seed"] for t in tr] == seeds
    want = _by_hand(s, pose, n_motion, seeds, steps, wo, remove, tea)
    for k in range(CLIPS):
        if k:
            assert torch.equal(tr[k]["motion"], tr[k - 1]["frames"][-n_motion:])
        if remove:
            assert tr[k]["add_condition"] is None
        else:
            assert torch.equal(tr[k]["add_condition"], want[k]["add_condition"]), k
        assert torch.equal(tr[k]["y"], want[k]["y"]), k
        assert torch.equal(tr[k]["latents"], want[k]["latents"]), k
        assert torch.equal(tr[k]["frames"], want[k]["frames"]), k
    assert torch.equal(video_u8, torch.cat([c["frames"][:-n_motion] for c in want[:-1]] + [want[-1]["frames"]]))
    # one resident loop: what was captured for clip 0 is what clips 1 and 2 replayed — the same count and the very same graph objects
    assert tr[0]["captures"] >= 1 and tr[2]["captures"] == tr[0]["captures"], [t["captures"] for t in tr]
    held = {id(g) for g in tr[0]["graphs"]}                   # (trace keeps the graph objects alive: an id is not reused)
    assert len(held) >= 1 and all({id(g) for g in t["graphs"]} == held for t in tr)
    if thresh is None:
        assert sl.loop.captures == 1
    if thresh == 1e9:
        assert sl.loop.tea_counts["skipped"] >= 1 and tr[0]["captures"] >= 2          # a computed step's graph and a skipped step's
    # the pose reaches the video, and the window moved: the clips' conditions differ (a stream without pose has none)
    if not remove:
        assert not torch.equal(tr[0]["add_condition"], tr[1]["add_condition"])
        table = frame_table(pose.shape[0], NF, n_motion, CLIPS)
        assert table[1] != table[0] and table[2] != table[1]
        if (n_motion, video) == (1, "long"):
            assert table[2][-1] == 0 and table[2][-2] == pose.shape[0] - 1                 # the cursor wrapped inside clip 2


def test_pose_changes_the_stream():
    """remove_pose and the two branch rules are three different streams (the condition is not dropped on the way into the resident loop)."""
    import svi_hip
    s = _shared()
    outs = []
    for kw in (dict(remove_pose=True), dict(cond_wo_pose=True), dict(cond_wo_pose=False)):
        sl = svi_hip.DanceStreamLoop(s["dit"], s["vae"], s["pose"], num_motion_frames=1, num_frames=NF, num_inference_steps=2, cfg_scale=SCALES, ref_pad_num=-1, **kw)
        sl.run(s["img"], s["ref_frame"], s["prompt"], s["long"], 2, seed=5, clip_feature=s["clipf"])
        outs.append(sl.trace[1]["latents"])
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2]) and not torch.equal(outs[0], outs[2])


def test_a_dance_stream_that_fails_midway_hands_the_model_back():
    """The clip encoder raises at clip 1, behind clip 0's capture and context cache: run() passes the error on and leaves neither; the same loop object
    then runs the stream as a newly built one does."""
    import svi_hip
    s, calls = _shared(), []

    def encoder(first):
        calls.append(first)
        if len(calls) == 2:
            raise RuntimeError("the clip encoder failed")
        return s["clipf"]
    mk = lambda enc: svi_hip.DanceStreamLoop(s["dit"], s["vae"], s["pose"], clip_encoder=enc, num_motion_frames=1, num_frames=NF,      # noqa: E731
                                             num_inference_steps=2, cfg_scale=SCALES, ref_pad_num=-1)
    sl = mk(encoder)
    with pytest.raises(RuntimeError, match="the clip encoder failed"):
        sl.run(s["img"], s["ref_frame"], s["prompt"], s["long"], 2, seed=5)
    assert len(calls) == 2 and len(sl.trace) == 1 and sl.trace[0]["captures"] == 1                      # clip 0 ran, on a captured step
    assert s["dit"]._ctx_cache_on is False and not s["dit"]._audio_slots and sl.loop.held_graphs() == []
    again = sl.run(s["img"], s["ref_frame"], s["prompt"], s["long"], 2, seed=5)
    fresh = mk(lambda first: s["clipf"]).run(s["img"], s["ref_frame"], s["prompt"], s["long"], 2, seed=5)
    assert len(calls) == 4 and tuple(again.shape) == (NF - 1 + NF, H, W, 3) and torch.equal(again, fresh)
    assert s["dit"]._ctx_cache_on is False


def test_dance_stream_refusals():
    import svi_hip
    s = _shared()
    mk = lambda **kw: svi_hip.DanceStreamLoop(s["dit"], s["vae"], kw.pop("pose", s["pose"]), **dict(dict(num_frames=NF, num_inference_steps=2), **kw))      # noqa: E731
    with pytest.raises(ValueError, match="4 k \\+ 1"):
        mk(num_frames=10)
    with pytest.raises(ValueError, match="num_motion_frames"):
        mk(num_motion_frames=0)
    with pytest.raises(ValueError, match="num_motion_frames"):
        mk(num_motion_frames=NF)
    with pytest.raises(ValueError, match="'text'"):
        mk(cfg_scale=dict(audio=1.0))
    wide = svi_hip.PoseEmbedder.from_state_dict({k: torch.from_numpy(v) for k, v in synth.pose_state_dict(synth.POSE_SEED, dim=256).items()})
    with pytest.raises(ValueError, match="dim 256 is not the DiT's dim 128"):
        mk(pose=wide)
    sl = mk(cfg_scale=SCALES)
    run = lambda pose, img=s["img"], **kw: sl.run(img, s["ref_frame"], s["prompt"], pose, 1, clip_feature=s["clipf"], **kw)      # noqa: E731
    with pytest.raises(ValueError, match="uint8 \\[N >= 1, h, w, 3\\]"):
        run(s["long"].float())
    with pytest.raises(ValueError, match="uint8 \\[N >= 1, h, w, 3\\]"):
        run(s["long"][..., :2])
    with pytest.raises(ValueError, match="uint8 \\[N >= 1, h, w, 3\\]"):
        run(s["long"][:0])
    with pytest.raises(ValueError, match="seeds"):
        sl.run(s["img"], s["ref_frame"], s["prompt"], s["long"], 2, seed=[1], clip_feature=s["clipf"])

    class Coarse:                                   # an embedder of the DiT's width whose token grid is not the DiT's
        dim = CFG["dim"]

        def tokens(self, F, H, W):
            return (TLAT, H // 32, W // 32)
    with pytest.raises(ValueError, match="token grid"):
        mk(pose=Coarse(), cfg_scale=SCALES).run(s["img"], s["ref_frame"], s["prompt"], s["long"], 1, clip_feature=s["clipf"])


def test_example_launcher_runs_a_synthetic_dance_stream(tmp_path):
    """examples/test_svi_dance_hip.py --synthetic: the reference CLI's surface over the whole chain on a box with no weights: 3 clips of 9 frames,
    stitched by the script's rule, pose windows 0 / 1 / 2, one captured step graph."""
    import json
    import os
    import subprocess
    import sys
    import numpy as np
    from conftest import ROOT
    script = os.path.join(ROOT, "examples", "test_svi_dance_hip.py")
    r = subprocess.run([sys.executable, script, "--synthetic", "--num_clips", "3", "--num_steps", "3", "--num_motion_frames", "2", "--output", str(tmp_path)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    rec = json.loads([l for l in r.stdout.splitlines() if l.startswith('{"test_svi_dance_hip"')][-1])["test_svi_dance_hip"][0]
    assert rec["clips"] == 3 and rec["frames"] == 2 * 7 + 9 and rec["pose_windows"] == [0, 1, 2] and rec["step_graph_captures"] == 1
    assert (rec["height"], rec["width"], rec["frames_per_clip"]) == (32, 48, 9) and rec["pose_frames"] < 3 * 9         # the stream outlasts its pose video
    vid = np.load(os.path.join(rec["out"], "video_u8.npy"))
    assert vid.shape == (23, 32, 48, 3) and vid.dtype == np.uint8 and vid.std() > 0
