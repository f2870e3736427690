"""The talk clip, three eager forwards per step against the one-call graphed step, in one process, alternating.

    python tools/talk3_ab.py [--sizes tiny,14b] [--steps 3] [--rounds 5] [--layers 4] [--commit ID]

Arm `eager`:  DenoiseLoop(graph=False).sample_multitalk — per step three model_fn_wan_talk_video calls (each re-runs the timestep embedding, the patch
              embedding, AudioProjModel, block 0's self-attention and every block's audio K / V^T projection) plus cfg3_step_.
Arm `talk3`:  DenoiseLoop(graph=True).sample_multitalk — both audio tuples staged into the DiT's audio slots once per clip, then per step one
              svi_dit_forward_talk3 call, captured on the clip's first step and replayed, plus cfg3_step_.
Sizes: `tiny` = the tiny talk model of the tests (dim 256, 2 layers, 3x4x6 tokens); `14b` = the 14B talk widths (dim 5120, ffn 13824, 40 heads) with
--layers blocks at the size the talk model runs (21 latent frames at 832x480: 32760 tokens, 512 prompt rows), random-init weights (bench.py's).
A clip is one sample_multitalk call between two HIP events (so staging, the eager first step and its capture count against the talk3 arm); the arms
alternate clip by clip after one untimed warm-up clip each, and their latents are compared bit for bit.  Nothing gates on these numbers: the one-call
step is the default because it puts the talk variant on the loop's one path, not because of a measured gain."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stable-video-infinity_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch      # noqa: E402

import bench      # noqa: E402
import svi_hip    # noqa: E402
import synth      # noqa: E402


def build(size, layers, dev):
    """-> (dit, (f, h, w) token grid, prompt rows)"""
    if size == "tiny":
        cfg, grid, lc = dict(synth.TINY_DIT_TALK), synth.TALK_GRID, 20
    else:
        cfg, grid, lc = dict(synth.WAN_14B_I2V, num_layers=layers, enable_multitalk=True), (21, 30, 52), 512
    dit = svi_hip.WanDiT(eps=1e-6, num_heads=cfg["dim"] // 128, **cfg)
    dit.bind(bench.device_weights(cfg, 0, dev))
    return dit, cfg, grid, lc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="tiny,14b")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--commit", default="(not given)")
    args = ap.parse_args()
    dev = torch.device("cuda")
    print(f"box: {torch.cuda.get_device_name(0)}; commit: {args.commit}; torch {torch.__version__}; random init; {args.steps} steps per clip, text scale 5, "
          f"audio scale 4; {args.rounds} rounds, arms alternating clip by clip")
    for size in args.sizes.split(","):
        dit, cfg, (f, h, w), lc = build(size, args.layers, dev)
        gen = torch.Generator(device=dev).manual_seed(1234)
        rnd = lambda *s, scale=1.0: (scale * torch.randn(s, generator=gen, device=dev)).to(torch.bfloat16)      # noqa: E731
        lat0 = svi_hip.generate_noise((1, 16, f, 2 * h, 2 * w), seed=0, device="cpu", dtype=torch.float32).to(dev, torch.bfloat16)
        cp, cn = rnd(1, lc, cfg["text_dim"]), rnd(1, lc, cfg["text_dim"])
        cp[:, min(64, lc - 4):] = 0
        cn[:, min(32, lc - 8):] = 0
        kw = dict(clip_feature=rnd(1, 257, 1280), y=rnd(1, cfg["in_dim"] - 16, f, 2 * h, 2 * w))
        aud = (rnd(1, 1, 5, 12, 768, scale=0.5), rnd(1, f - 1, 8, 12, 768, scale=0.5))
        null = (torch.zeros_like(aud[0]), torch.zeros_like(aud[1]))
        arms = {"eager": svi_hip.DenoiseLoop(dit, graph=False), "talk3": svi_hip.DenoiseLoop(dit, graph=True)}
        out, clips = {}, {a: [] for a in arms}
        for r in range(args.rounds + 1):                           # round 0 warms both arms up, untimed
            for name in (("eager", "talk3") if r % 2 else ("talk3", "eager")):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                out[name] = arms[name].sample_multitalk(lat0, cp, cn, aud, null, num_inference_steps=args.steps, text_scale=5.0, audio_scale=4.0, **kw)
                e1.record()
                torch.cuda.synchronize()
                if r:
                    clips[name].append(e0.elapsed_time(e1))
        same = bool(torch.equal(out["eager"], out["talk3"]))
        print(f"\n{size}: dim {cfg['dim']}, {cfg['num_layers']} layers, {f}x{h}x{w} = {f * h * w} tokens, {lc} prompt rows; talk3 latents == eager latents: {same}")
        print(f"  {'arm':6s} {'clip ms':>10s} {'per step':>10s}   (median of {args.rounds} clips; min..max)")
        for name in arms:
            c = clips[name]
            print(f"  {name:6s} {statistics.median(c):10.2f} {statistics.median(c) / args.steps:10.2f}   {min(c):.2f}..{max(c):.2f}")
        me, mt = statistics.median(clips["eager"]), statistics.median(clips["talk3"])
        print(f"  talk3 / eager = {mt / me:.4f}  ({100.0 * (me - mt) / me:+.2f} % of the eager clip saved; captures per clip: {arms['talk3'].captures / (args.rounds + 1):.0f})")
        arms["talk3"].release()
        del arms, dit
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
