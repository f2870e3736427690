"""TeaCache steps, eager against graphed, in one process, alternating (the question of DESIGN §4's TeaCache paragraph).

    python tools/teacache_graph_ab.py [--sizes c1,c2] [--steps 10] [--rounds 5] [--thresh 0.3] [--commit ID]

Arm `eager`:  DenoiseLoop(graph=False) — each branch of a step through model_fn_wan_video: two svi_dit_forward_tea calls, a decision read-back per branch.
Arm `graph`:  DenoiseLoop(graph=True)  — the decisions first, then one svi_dit_forward_cfg_pair_tea call per step, captured once per mode and replayed.
Wan2.1-T2V-1.3B widths, random-init weights (bench.py's), CFG 5, the C1 size (17 frames at 256x256) and the C2 size (81 frames at 832x480).
Every step is timed with a pair of HIP events around DenoiseLoop.step (so the host's part of a launch-bound step counts); a clip is one sample()-like
pass.  Reported per arm and size: the median over all rounds of a computed step, of a skipped step, of the steps that also captured their graph (graph
arm, non-resident: one computed and one skipped step per clip — the eager run plus its recording), and of the whole clip; the arms alternate clip by
clip after one untimed warm-up clip each, and their latents are compared bit for bit.  The last lines say whether the graphed path earned the default
(lower clip median at BOTH sizes) or stays opt-in."""
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
from svi_hip.teacache import TeaCache      # noqa: E402

MODEL_ID = "Wan2.1-T2V-1.3B"
KINDS = ("computed", "skipped", "computed capture", "skipped capture")      # "... capture": the step also captured its graph (the eager run plus its recording)


class NotingTeaCache(TeaCache):
    """svi_hip.TeaCache that also notes its decisions (the eager arm keeps no counters)."""
    def __init__(self, *a):
        super().__init__(*a)
        self.pattern = []

    def check(self, dit, x, t_mod):
        skip = super().check(dit, x, t_mod)
        self.pattern.append(skip)
        return skip


def clip(loop, lat0, cp, cn, steps, thresh):
    """One clip as DenoiseLoop.sample runs it, with every step between two events.  -> (latents, [(kind, ms)], clip ms, skip pattern)"""
    loop.scheduler.set_timesteps(steps, shift=5.0)
    ts = loop.scheduler.timesteps.to(lat0.device, torch.float32)
    tp, tn = NotingTeaCache(steps, thresh, MODEL_ID), NotingTeaCache(steps, thresh, MODEL_ID)
    lat = lat0.clone()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    kinds = []
    loop.dit.context_cache(True)
    try:
        torch.cuda.synchronize()
        ev[0].record()
        for i, t in enumerate(loop.scheduler.timesteps):
            caps = loop.captures
            loop.step(lat, ts[i:i + 1], loop.scheduler.step_delta(t), cp, cn, 5.0, tea_cache_posi=tp, tea_cache_nega=tn)
            ev[i + 1].record()
            kinds.append(("skipped" if tp.pattern[i] else "computed") + (" capture" if loop.captures != caps else ""))
        torch.cuda.synchronize()
    finally:
        loop.drop_graph()
        loop.dit.context_cache(False)
    ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(steps)]
    return lat, list(zip(kinds, ms)), ev[0].elapsed_time(ev[steps]), "".join("S" if s else "C" for s in tp.pattern)


def med(v):
    return statistics.median(v) if v else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="c1,c2")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--thresh", type=float, default=0.3)
    ap.add_argument("--commit", default="(not given)")
    args = ap.parse_args()
    dev = torch.device("cuda")
    cfg = dict(synth.WAN_1_3B)
    dit = svi_hip.WanDiT(eps=1e-6, num_heads=cfg["dim"] // 128, **cfg)
    dit.bind(bench.device_weights(cfg, 0, dev))
    print(f"box: {torch.cuda.get_device_name(0)}; commit: {args.commit}; torch {torch.__version__}; model {MODEL_ID} widths, random init; "
          f"threshold {args.thresh}; {args.steps} steps per clip; {args.rounds} rounds, arms alternating clip by clip")
    verdict = []
    for size in args.sizes.split(","):
        wl = bench.WORKLOADS[size]
        T, H, W = wl["lat"]
        gen = torch.Generator(device=dev).manual_seed(1234)
        lat0 = svi_hip.generate_noise((1, 16, T, H, W), seed=0, device="cpu", dtype=torch.float32).to(dev, torch.bfloat16)
        cp = torch.randn((1, wl["lc"], 4096), generator=gen, device=dev).to(torch.bfloat16)
        cn = torch.randn((1, wl["lc"], 4096), generator=gen, device=dev).to(torch.bfloat16)
        cp[:, 64:] = 0
        cn[:, 32:] = 0
        arms = {"eager": svi_hip.DenoiseLoop(dit, graph=False), "graph": svi_hip.DenoiseLoop(dit, graph=True)}
        out, per, clips, pattern = {}, {a: {k: [] for k in KINDS} for a in arms}, {a: [] for a in arms}, None
        for rnd in range(args.rounds + 1):                         # round 0 warms both arms up, untimed
            for name in (("eager", "graph") if rnd % 2 else ("graph", "eager")):
                lat, steps, total, pat = clip(arms[name], lat0, cp, cn, args.steps, args.thresh)
                out[name], pattern = lat, pat
                if rnd:
                    clips[name].append(total)
                    for kind, ms in steps:
                        per[name][kind].append(ms)
        same = bool(torch.equal(out["eager"], out["graph"]))
        print(f"\n{size}: latents {T}x{H}x{W}, {wl['lc']} prompt rows; decisions {pattern}; graphed latents == eager latents: {same}")
        print(f"  {'arm':6s} {'computed ms':>12s} {'skipped ms':>11s} {'computed+capture':>17s} {'skipped+capture':>16s} {'clip ms':>9s}   (medians; n per column)")
        for name in arms:
            p = per[name]
            print(f"  {name:6s} {med(p[KINDS[0]]):12.3f} {med(p[KINDS[1]]):11.3f} {med(p[KINDS[2]]):17.3f} {med(p[KINDS[3]]):16.3f} {med(clips[name]):9.2f}   "
                  f"n = {'/'.join(str(len(p[k])) for k in KINDS)}/{len(clips[name])}; clip min..max {min(clips[name]):.2f}..{max(clips[name]):.2f}")
        verdict.append((size, med(clips["graph"]) < med(clips["eager"]), same))
        arms["graph"].release()
    on = all(v[1] for v in verdict) and len(verdict) == 2
    print("\nclip median lower with graph=True: " + ", ".join(f"{s}: {'yes' if lower else 'no'}" for s, lower, _ in verdict))
    print(f"bit-identical at every size: {all(v[2] for v in verdict)}")
    print("decision: TeaCache under graph=None " + ("takes the graphed path (TEA_GRAPH_BY_DEFAULT = True)" if on else
                                                      "stays on the eager path; graph=True opts in (TEA_GRAPH_BY_DEFAULT = False)"))


if __name__ == "__main__":
    main()
