"""A talk clip with TeaCache: the eager three-forward loop with the cache objects against the one-call graphed step, in one process, alternating.

    python tools/talk3_tea_ab.py [--sizes tiny,14b] [--steps 10] [--rounds 4] [--layers 4] [--commit ID]

Arm `eager`:  DenoiseLoop(graph=False).sample_multitalk(tea_cache_l1_thresh=...) — what a TeaCache talk clip ran on before the one-call step took it: per
              step three model_fn_wan_talk_video(tea_cache=...) calls (positive object, then the negative object twice), each re-running the timestep
              and patch embedding, and — where it computes — AudioProjModel and every block's audio K / V^T projection; no graph.
Arm `talk3`:  DenoiseLoop(graph=True).sample_multitalk(tea_cache_l1_thresh=...) — the three decisions on the host, then one svi_dit_forward_talk3_tea call
              replayed from the graph of its mode triple, audio slots staged once per clip.
Sizes as tools/talk3_ab.py: `tiny` = the tests' talk model; `14b` = the 14B talk widths with --layers blocks at 32760 tokens, random-init weights.
Threshold: the random time embedding makes the per-step drift of the model id's polynomial arbitrary, so it is MEASURED first (the positive object's
increments over the schedule, host arithmetic on svi_dit_time_mod) and the threshold is set to 2.5 x their median: about two skipped steps per computed
one, both kinds of step present; the per-triple step counts are printed.  A clip is one sample_multitalk call between two HIP events (staging, eager
first steps and captures count against the talk3 arm); the arms alternate clip by clip after one untimed warm-up clip each; latents compared bit for
bit.  Nothing gates on these numbers."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stable-video-infinity_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch      # noqa: E402

import svi_hip    # noqa: E402
from talk3_ab import build      # noqa: E402

MODEL_ID = "Wan2.1-I2V-14B-480P"


def pick_threshold(dit, steps):
    """2.5 x the median per-step increment of a TeaCache object that never resets, over this model's own t_mod on the clip's schedule."""
    sch = svi_hip.FlowMatchScheduler(shift=5, sigma_min=0.0, extra_one_step=True)
    sch.set_timesteps(steps, shift=5.0)
    probe = svi_hip.TeaCache(steps, float("inf"), MODEL_ID)
    inc = []
    for t in sch.timesteps[:-1]:
        before = probe.accumulated_rel_l1_distance
        probe.check(dit, None, dit.time_mod(t.reshape(1)))
        inc.append(probe.accumulated_rel_l1_distance - before)
    return 2.5 * statistics.median(inc[1:]), inc[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="tiny,14b")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--commit", default="(not given)")
    args = ap.parse_args()
    dev = torch.device("cuda")
    print(f"box: {torch.cuda.get_device_name(0)}; commit: {args.commit}; torch {torch.__version__}; random init; {args.steps} steps per clip, text scale 5, "
          f"audio scale 4, TeaCache model id {MODEL_ID}; {args.rounds} rounds, arms alternating clip by clip")
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
        thresh, inc = pick_threshold(dit, args.steps)
        arms = {"eager": svi_hip.DenoiseLoop(dit, graph=False), "talk3": svi_hip.DenoiseLoop(dit, graph=True)}
        out, clips = {}, {a: [] for a in arms}
        for r in range(args.rounds + 1):                           # round 0 warms both arms up, untimed
            for name in (("eager", "talk3") if r % 2 else ("talk3", "eager")):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                out[name] = arms[name].sample_multitalk(lat0, cp, cn, aud, null, num_inference_steps=args.steps, text_scale=5.0, audio_scale=4.0,
                                                        tea_cache_l1_thresh=thresh, tea_cache_model_id=MODEL_ID, **kw)
                e1.record()
                torch.cuda.synchronize()
                if r:
                    clips[name].append(e0.elapsed_time(e1))
        same = bool(torch.equal(out["eager"], out["talk3"]))
        counts = arms["talk3"].talk_tea_counts
        print(f"\n{size}: dim {cfg['dim']}, {cfg['num_layers']} layers, {f}x{h}x{w} = {f * h * w} tokens, {lc} prompt rows; talk3 latents == eager latents: {same}")
        print(f"  threshold {thresh:.4g} (per-step increments {min(inc):.4g} .. {max(inc):.4g}); steps per mode triple (cond, uncond, drop-text; 1 = computed, "
              f"2 = skipped): {', '.join(f'{t}: {n}' for t, n in sorted(counts.items()))}")
        print(f"  {'arm':6s} {'clip ms':>10s} {'per step':>10s}   (median of {args.rounds} clips; min..max)")
        for name in arms:
            c = clips[name]
            print(f"  {name:6s} {statistics.median(c):10.2f} {statistics.median(c) / args.steps:10.2f}   {min(c):.2f}..{max(c):.2f}")
        me, mt = statistics.median(clips["eager"]), statistics.median(clips["talk3"])
        print(f"  talk3 / eager = {mt / me:.4f}  ({100.0 * (me - mt) / me:+.2f} % of the eager clip saved; captures per clip: "
              f"{arms['talk3'].captures / (args.rounds + 1):.1f})")
        arms["talk3"].release()
        del arms, dit
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
