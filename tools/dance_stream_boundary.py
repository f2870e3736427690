"""The clip boundary of a dance stream: the host path a caller had to write against the device path of DanceStreamLoop, in one process, alternating.

    python tools/dance_stream_boundary.py [--rounds 10] [--pose_frames 200] [--commit ID] [--out profiles/dance_stream_boundary.txt]

Arm `host`:   what the reference's script does between two clips (test_svi_dance.py:281-288) on the pose video it resized ONCE up front (:215, not timed
              here): the window's frames gathered on the host into a float32 [3, 81, 480, 832] tensor, its upload (388 MB), PoseEmbedder.__call__.
Arm `device`: PoseEmbedder.window on the 8-bit pose video resident at its source resolution: svi_pose_window into the embedder's window buffer, then
              the same embedder launches.
Sizes: 81 frames of 480 x 832 from a 1080 x 1920 source, one motion frame, the 14B width (dim 5120), random init; the clip index walks on as the stream's
does.  Each boundary is timed twice: HIP events around it on the stream, and the host's wall clock from before the call to after a synchronize.  The arms
alternate boundary by boundary after one untimed warm-up each; the two conditions are compared bit for bit once.  The window kernel alone is timed as
--reps launches between one pair of events into one buffer; its bytes are counted from the shapes.  Nothing gates on these numbers."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "stable-video-infinity_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch      # noqa: E402

import svi_hip    # noqa: E402
import synth      # noqa: E402
from dance_stream_cases import frame_table, resize_pad, scaled_size      # noqa: E402

F, H, W, MOTION, SRC_H, SRC_W, DIM = 81, 480, 832, 1, 1080, 1920, 5120
HBM_BYTES_PER_S = 8.0e12          # the figure DESIGN.md uses for the part


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
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--pose_frames", type=int, default=200)
    ap.add_argument("--commit", default="(not given)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    N = args.pose_frames
    g = torch.Generator().manual_seed(5)
    pose_host = torch.randint(0, 256, (N, SRC_H, SRC_W, 3), generator=g, dtype=torch.uint8) * (torch.rand((N, SRC_H, SRC_W, 1), generator=g) < 0.3)
    pose_dev = pose_host.to(dev)
    resized = torch.cat([resize_pad(pose_host[i:i + 20], H, W) for i in range(0, N, 20)])      # the script's one-off resize of the whole video: uint8 [N, H, W, 3]
    emb = svi_hip.PoseEmbedder.from_state_dict({k: torch.from_numpy(v) for k, v in synth.pose_state_dict(synth.POSE_SEED, dim=DIM).items()}, device=dev)
    clips = args.rounds + 2
    table = frame_table(N, F, MOTION, clips)
    say(f"box: {torch.cuda.get_device_name(0)}; commit: {args.commit}; torch {torch.__version__}; random init; pose video uint8 [{N}, {SRC_H}, {SRC_W}, 3] "
        f"({pose_host.numel() / 1e9:.2f} GB resident); window fp32 [3, {F}, {H}, {W}]; embedder dim {DIM}; {args.rounds} boundaries per arm, alternating")

    def host_boundary(k):
        window = torch.zeros((3, F, H, W), dtype=torch.float32)
        window[:] = resized[table[k]].permute(3, 0, 1, 2)                          # the gather and the float conversion
        return emb(window.to(dev))

    def device_boundary(k):
        return emb.window(pose_dev, k, F, MOTION, H, W)
    a, b = host_boundary(1), device_boundary(1)
    say(f"add_condition of clip 1, device path == host path: {torch.equal(a, b)}  ({tuple(a.shape)} bf16)")
    arms = {"host": host_boundary, "device": device_boundary}
    ev, wall = {k: [] for k in arms}, {k: [] for k in arms}
    for r in range(args.rounds + 1):
        for name in (("host", "device") if r % 2 else ("device", "host")):
            e, t = timed(lambda: arms[name](r + 1))
            if r:
                ev[name].append(e)
                wall[name].append(t)
    say(f"\n  {'arm':8s} {'events ms':>10s} {'min..max':>20s} {'wall ms':>10s} {'min..max':>20s}   (median of {args.rounds} boundaries)")
    for name in arms:
        say(f"  {name:8s} {statistics.median(ev[name]):10.3f} {min(ev[name]):9.3f}..{max(ev[name]):<9.3f} {statistics.median(wall[name]):10.3f} "
            f"{min(wall[name]):9.3f}..{max(wall[name]):<9.3f}")
    say(f"  device / host (wall) = {statistics.median(wall['device']) / statistics.median(wall['host']):.4f}; "
        f"(events) = {statistics.median(ev['device']) / statistics.median(ev['host']):.4f}")
    # ---- the host path's parts (wall clock, median)
    gather, upload = [], []
    for r in range(args.rounds):
        t0 = time.perf_counter()
        window = torch.zeros((3, F, H, W), dtype=torch.float32)
        window[:] = resized[table[r + 1]].permute(3, 0, 1, 2)
        t1 = time.perf_counter()
        window.to(dev)
        torch.cuda.synchronize()
        gather.append((t1 - t0) * 1e3)
        upload.append((time.perf_counter() - t1) * 1e3)
    say(f"  host gather + float conversion alone: {statistics.median(gather):.3f} ms; upload of {3 * F * H * W * 4 / 1e6:.1f} MB alone: {statistics.median(upload):.3f} ms")
    # ---- the embedder alone and the window kernel alone
    buf = torch.empty((3, F, H, W), dtype=torch.float32, device=dev)
    svi_hip.pose_window(pose_dev, 1, F, MOTION, H, W, out=buf)
    ms, _ = timed(lambda: [emb(buf) for _ in range(5)])
    say(f"  PoseEmbedder.__call__ alone: {ms / 5:.3f} ms (5 calls between two events)")
    ms, _ = timed(lambda: [svi_hip.pose_window(pose_dev, 1 + i % clips, F, MOTION, H, W, out=buf) for i in range(args.reps)])
    us = ms * 1e3 / args.reps
    nh, nw, _, _ = scaled_size(SRC_H, SRC_W, H, W)
    written, read = 3 * F * H * W * 4, F * nh * nw * 3
    say(f"  svi_pose_window alone: {us:.2f} us per launch ({args.reps} launches between two events, into one buffer); written 3 x {F} x {H} x {W} x 4 B = {written} B, "
        f"source pixels read {F} x {nh} x {nw} x 3 B = {read} B (the cache lines they lie in: more) -> {(written + read) / (us * 1e-6) / 1e12:.3f} TB/s "
        f"= {100 * (written + read) / (us * 1e-6) / HBM_BYTES_PER_S:.1f} % of {HBM_BYTES_PER_S / 1e12:.0f} TB/s")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
