"""The talk variant on sequence shards, timed on ONE GPU with HIP events (A and B alternate within the job):

  (a) one block's audio cross-attention at the 14B talk width (dim 5120, 40 heads) on the 21 x 30 x 52 latent grid (32760 rows, 1560 per frame,
      32 audio tokens per frame): the 21 per-frame launches the DiT made before (svi_attention_vt_fwd, one per frame) against the one
      frame-segmented launch (svi_attention_frames_fwd) — and whether the two give the same bits;
  (b) the talk forward of a few-block Wan2.1-I2V-14B model with enable_multitalk, single rank (model_fn_wan_talk_video) against P = 2, 4, 8 shards run
      back to back in this process (sequence_parallel.forward_local, the exchange as device copies); per rank = all shards / P, i.e. the
      per-rank compute plus its share of the simulated transport, before any real interconnect.

    python tools/talk_sp_timing.py [--layers 3] [--reps 5] [--out profiles/talk_sp_timing.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stable-video-infinity_amd")); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import torch  # noqa: E402

import svi_hip  # noqa: E402
import synth  # noqa: E402
from svi_hip import _lib as L  # noqa: E402
from svi_hip import sequence_parallel as sp  # noqa: E402
from bench import device_weights  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=3)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "talk_sp_timing.txt"))
args = ap.parse_args()
assert torch.cuda.is_available(), "talk_sp_timing.py measures on the GPU"
dev = torch.device("cuda")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(fn, n=1):
    """ms per call of fn over n back-to-back calls, HIP events on the current stream."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def alternate(fns, reps, n=1):
    """Warm every candidate, then time them in turn, `reps` rounds: name -> list of ms."""
    for f in fns.values():
        f(); torch.cuda.synchronize()
    got = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            got[k].append(timed(f, n))
    return got


def summary(ms):
    return f"median {statistics.median(ms):8.3f} ms  min {min(ms):8.3f}  max {max(ms):8.3f}"


say(f"device: {torch.cuda.get_device_name(0)}; reps {args.reps} (alternating)")

# ---- (a) one block's audio attention ------------------------------------------------------------------------------------------------
D, H, KPF = 5120, 40, 32
f, hh, ww = 21, 30, 52
rpf, Lt = hh * ww, f * hh * ww
g = torch.Generator(device=dev).manual_seed(7)
qk = torch.randn((Lt, 2 * D), generator=g, device=dev).to(torch.bfloat16)         # q in the DiT's q | k buffer: row stride 2 D
k = torch.randn((f * KPF, D), generator=g, device=dev).to(torch.bfloat16)
vt = torch.randn((D, f * KPF), generator=g, device=dev).to(torch.bfloat16)
o_a, o_b = torch.empty((Lt, D), dtype=torch.bfloat16, device=dev), torch.empty((Lt, D), dtype=torch.bfloat16, device=dev)
lib = L.lib()


def per_frame():
    st = L.current_stream()
    for fr in range(f):
        L.check(lib.svi_attention_vt_fwd(qk.data_ptr() + fr * rpf * 2 * D * 2, 2 * D, k.data_ptr() + fr * KPF * D * 2, D, vt.data_ptr() + fr * KPF * 2,
                                         vt.shape[1], o_a.data_ptr() + fr * rpf * D * 2, D, rpf, KPF, H, 0, st), "svi_attention_vt_fwd")


def one_launch():
    L.check(lib.svi_attention_frames_fwd(qk.data_ptr(), 2 * D, k.data_ptr(), D, vt.data_ptr(), vt.shape[1], o_b.data_ptr(), D, 0, Lt, rpf, KPF, H,
                                         L.current_stream()), "svi_attention_frames_fwd")


res = alternate({"per-frame": per_frame, "frames": one_launch}, args.reps, n=20)
say()
say(f"(a) audio attention of one block, dim {D}, {H} heads, grid {f}x{hh}x{ww} ({Lt} rows, {rpf} per frame, {KPF} keys per frame); 20 calls per sample")
say(f"    {f} per-frame launches (before): {summary(res['per-frame'])}")
say(f"    one frame-segmented launch:      {summary(res['frames'])}")
say(f"    ratio of medians (one / per-frame): {statistics.median(res['frames']) / statistics.median(res['per-frame']):.3f}; "
    f"same bits: {bool(torch.equal(o_a, o_b))}")
bytes_moved = Lt * D * 2 * 2 + H * f * KPF * 128 * 2 * 2
say(f"    q read + o written + K / V^T: {bytes_moved / 1e6:.0f} MB -> {bytes_moved / statistics.median(res['frames']) / 1e9:.2f} TB/s for the one launch")
del qk, k, vt, o_a, o_b

# ---- (b) the talk forward on shards -------------------------------------------------------------------------------------------------
cfg = dict(synth.WAN_14B_I2V, enable_multitalk=True, num_layers=args.layers)
sd = device_weights(cfg, 0, dev)


def handle():
    m = svi_hip.WanDiT(eps=1e-6, num_heads=cfg["dim"] // 128, **cfg)
    m.bind(sd)
    m.context_cache(True)                       # as DenoiseLoop.sample_multitalk runs it
    return m


g = torch.Generator(device=dev).manual_seed(11)
x = torch.randn((1, 16, f, 2 * hh, 2 * ww), generator=g, device=dev).to(torch.bfloat16)
y = torch.randn((1, 20, f, 2 * hh, 2 * ww), generator=g, device=dev).to(torch.bfloat16)
clip = torch.randn((1, 257, 1280), generator=g, device=dev).to(torch.bfloat16)
ctx = torch.randn((1, 512, 4096), generator=g, device=dev).to(torch.bfloat16)
aud = ((0.5 * torch.randn((1, 1, 5, 12, 768), generator=g, device=dev)).to(torch.bfloat16),
       (0.5 * torch.randn((1, f - 1, 8, 12, 768), generator=g, device=dev)).to(torch.bfloat16))
t = torch.tensor([500.0])
single = handle()
shards = [handle() for _ in range(8)]
kw = dict(clip_feature=clip, y=y)
fns = {"single": lambda: svi_hip.model_fn_wan_talk_video(single, x, t, ctx, audio_embed_tuple=aud, **kw)}
for P in (2, 4, 8):
    fns[P] = (lambda P=P: sp.forward_local(shards[:P], x, t, ctx, audio_embed_tuple=aud, **kw))
res = alternate(fns, args.reps)
want = fns["single"]().clone()
say()
say(f"(b) talk forward, Wan2.1-I2V-14B widths + enable_multitalk, {args.layers} blocks, grid {f}x{hh}x{ww} ({Lt} tokens), prompt 512 tokens, context cache on")
base = statistics.median(res["single"])
say(f"    single rank (model_fn_wan_talk_video):   {summary(res['single'])}")
for P in (2, 4, 8):
    med = statistics.median(res[P])
    same = bool(torch.equal(fns[P](), want))
    say(f"    P={P} shards back to back (forward_local): {summary(res[P])}; per rank {med / P:8.3f} ms = {med / base:.3f} x (single-rank forward / P); "
        f"same bits as the single rank: {same}")

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
print(f"wrote {args.out}")
