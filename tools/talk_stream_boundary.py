"""The clip boundary of a talk stream: the host path it had against the device path of TalkStreamLoop, in one process, alternating.

    python tools/talk_stream_boundary.py [--layers 4] [--rounds 20] [--audio_frames 2000] [--commit ID] [--out profiles/talk_stream_boundary.txt]

Arm `host`:    what a talk clip boundary cost before: on the host, the [frames, 5] index table, the fancy-index gather over the fp32 embedding
               [N, 12, 768] and the six rearrange / concat passes of the reference (tests/audio_window_cases.py windows_einops), the null tuple, the cast
               to bf16, then WanDiT.stage_audio for both slots (which uploads the tuples and projects them).
Arm `windows`: WanDiT.stage_audio_windows on the embedding resident on the device: one svi_dit_audio_slot_windows call per slot (cut + projection).
Model: the 14B talk widths with --layers blocks (tools/talk3_ab.py's), random init; 21 latent frames (81 video frames); the cursor walks the stream as
TalkStreamLoop's does.  Each boundary is timed twice: HIP events around it on the stream, and the host's wall clock from before the call to after a
synchronize.  The arms alternate boundary by boundary after one untimed warm-up each; forward_talk3 on the two stagings is compared bit for bit once.
The cut kernel alone (svi_audio_windows, fp32 and bf16 source) is timed as 50 launches between one pair of events; its byte count is written out.
Nothing gates on these numbers."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stable-video-infinity_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import torch      # noqa: E402

import svi_hip    # noqa: E402
from audio_window_cases import windows_einops      # noqa: E402
from talk3_ab import build      # noqa: E402

T_LATENT, NUM_FRAMES, MOTION = 21, 81, 1
HBM_BYTES_PER_S = 8.0e12          # the figure DESIGN.md uses for the part


def host_boundary(dit, emb_host, start):
    first, latter = windows_einops(emb_host, start, T_LATENT)
    aud = (first, latter)
    null = (torch.zeros_like(first), torch.zeros_like(latter))
    dit.stage_audio(0, aud)
    dit.stage_audio(1, null)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--audio_frames", type=int, default=2000)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    dit, cfg, (f, h, w), lc = build("14b", args.layers, dev)
    assert f == T_LATENT
    N = args.audio_frames
    emb_host = 0.5 * torch.randn((N, 12, 768), generator=torch.Generator().manual_seed(5))
    emb_dev = emb_host.to(dev)
    say(f"box: {torch.cuda.get_device_name(0)}; commit: {args.commit}; torch {torch.__version__}; random init; dim {cfg['dim']}, {cfg['num_layers']} blocks; "
        f"embedding [{N}, 12, 768] fp32; {T_LATENT} latent frames; {args.rounds} boundaries per arm, alternating")
    # ---- the two stagings give the same forward_talk3, bit for bit
    gen = torch.Generator(device=dev).manual_seed(1234)
    rnd = lambda *s: torch.randn(s, generator=gen, device=dev).to(torch.bfloat16)      # noqa: E731
    x, cp, cn = rnd(1, 16, f, 2 * h, 2 * w), rnd(1, lc, cfg["text_dim"]), rnd(1, lc, cfg["text_dim"])
    kw = dict(clip_feature=rnd(1, 257, 1280), y=rnd(1, cfg["in_dim"] - 16, f, 2 * h, 2 * w))
    ts = torch.tensor([637.5], device=dev)
    host_boundary(dit, emb_host, 80)
    a = dit.forward_talk3(x, ts, cp, cn, **kw)
    dit.stage_audio_windows(emb_dev, 80, T_LATENT)
    b = dit.forward_talk3(x, ts, cp, cn, **kw)
    say(f"forward_talk3 after stage_audio_windows == after the host path + stage_audio: {all(torch.equal(p, q) for p, q in zip(a, b))}")
    # ---- the boundary, alternating
    arms = {"host": lambda s: host_boundary(dit, emb_host, s), "windows": lambda s: dit.stage_audio_windows(emb_dev, s, T_LATENT)}
    ev, wall = {k: [] for k in arms}, {k: [] for k in arms}
    for r in range(args.rounds + 1):
        start = (r * NUM_FRAMES - (MOTION if r else 0)) % max(N - NUM_FRAMES, 1)
        for name in (("host", "windows") if r % 2 else ("windows", "host")):
            e, t = timed(lambda: arms[name](start))
            if r:
                ev[name].append(e)
                wall[name].append(t)
    say(f"\n  {'arm':8s} {'events ms':>10s} {'min..max':>18s} {'wall ms':>10s} {'min..max':>18s}   (median of {args.rounds} boundaries)")
    for name in arms:
        say(f"  {name:8s} {statistics.median(ev[name]):10.3f} {min(ev[name]):8.3f}..{max(ev[name]):<8.3f} {statistics.median(wall[name]):10.3f} "
            f"{min(wall[name]):8.3f}..{max(wall[name]):<8.3f}")
    me, mw = statistics.median(wall["host"]), statistics.median(wall["windows"])
    say(f"  windows / host (wall) = {mw / me:.4f}; (events) = {statistics.median(ev['windows']) / statistics.median(ev['host']):.4f}")
    # ---- the host path's parts (wall clock, median): gather + regroup + cast on the host, and the rest (upload + projection of both slots)
    parts = []
    for r in range(args.rounds):
        t0 = time.perf_counter()
        first, latter = windows_einops(emb_host, r * NUM_FRAMES % (N - NUM_FRAMES), T_LATENT)
        parts.append((time.perf_counter() - t0) * 1e3)
    say(f"  host gather + regroup + cast alone: {statistics.median(parts):.3f} ms; upload of both tuples: "
        f"{2 * (5 + 8 * (T_LATENT - 1)) * 12 * 768 * 2 / 1e6:.2f} MB")
    # ---- the cut kernel alone
    rows = 5 + 8 * (T_LATENT - 1)
    for name, e in (("fp32", emb_dev), ("bf16", emb_dev.to(torch.bfloat16))):
        svi_hip.audio_windows(e, 80, T_LATENT)
        reps = 50
        ms, _ = timed(lambda: [svi_hip.audio_windows(e, 80 + i, T_LATENT) for i in range(reps)])
        us = ms * 1e3 / reps
        nbytes = rows * 12 * 768 * (e.element_size() + 2)
        say(f"  svi_audio_windows, {name} source: {us:.2f} us per launch (with its two output allocations; {reps} launches between two events); "
            f"{rows} rows x 9216 x ({e.element_size()} B read + 2 B written) = {nbytes} B -> {nbytes / (us * 1e-6) / 1e12:.3f} TB/s "
            f"= {100 * nbytes / (us * 1e-6) / HBM_BYTES_PER_S:.1f} % of {HBM_BYTES_PER_S / 1e12:.0f} TB/s")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
