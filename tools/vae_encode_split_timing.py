"""One rank's share of the exact VAE encode split next to the whole encode, on ONE GPU: the whole encode at [3, 81, 480, 832] alternated with each part
of a 1x2, 2x2 and 2x4 split (WanVideoVAE.encode_part into a tight buffer, as a rank of the latency modes would run it) and with the tail every rank
runs on the assembled feature map (WanVideoVAE.encode_tail).  Every timing sits between HIP events after a warm-up of the same call.  These are
per-part times of one device, not a scaling run: no all-gather, no second GPU.
    python tools/vae_encode_split_timing.py [--out profiles/vae_encode_split_timing.txt] [--small]
Reports ms for the whole encode, ms per part, the tail, and whole / (slowest part + tail), next to the ratio of pixel counts (whole video /
largest crop), which ignores the replicated tail."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stable-video-infinity_amd"))
import torch
from svi_hip import _lib
from svi_hip.vae import WanVideoVAE, device_vae_weights, encoder_feature_channels

args = sys.argv[1:]
out_path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "vae_encode_split_timing.txt")
shape = (3, 5, 160, 192) if "--small" in args else (3, 81, 480, 832)

dev = torch.device("cuda")
vae = WanVideoVAE.from_state_dict(device_vae_weights(0, dev))
video = torch.tanh(torch.randn(shape, generator=torch.Generator(device=dev).manual_seed(3), device=dev))
hh, ww, tl = shape[2] // 8, shape[3] // 8, 1 + (shape[1] - 1) // 4


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); out = fn(); e1.record(); torch.cuda.synchronize()
    del out
    return e0.elapsed_time(e1)


whole = lambda: vae.encode([video], device=dev)      # noqa: E731
timed(whole)                                         # warm-up: pool, LDS attributes, weight packing
feat = torch.empty((tl, hh, ww, encoder_feature_channels()), device=dev)
vae.encode_part(video, (1, 1), 0, out=feat)          # a real feature map for the tail
tail = lambda: vae.encode_tail(feat)                 # noqa: E731
timed(tail)
lines = [f"VAE encode split timing, video {list(shape)}, one GPU ({torch.cuda.get_device_name(0)}): per-part times, not a scaling run", ""]
for split in ((1, 2), (2, 2), (2, 4)):
    n = split[0] * split[1]
    whole_ms, part_ms, tail_ms = [], [], []
    for p in range(n):
        part = lambda p=p: vae.encode_part(video, split, p)      # noqa: E731
        timed(part)                                  # warm-up of this part's shapes
        whole_ms.append(timed(whole))
        part_ms.append(timed(part))
        tail_ms.append(timed(tail))
    w, t = sorted(whole_ms)[len(whole_ms) // 2], sorted(tail_ms)[len(tail_ms) // 2]
    slow = max(part_ms)
    plans = [_lib.vae_encode_split_plan(hh, ww, *split, p) for p in range(n)]
    crop = max((pl["rects"][0][1] - pl["rects"][0][0]) * (pl["rects"][0][3] - pl["rects"][0][2]) for pl in plans)
    lines.append(f"split {split[0]}x{split[1]}: whole {w:8.1f} ms (median of {n}, min {min(whole_ms):.1f} max {max(whole_ms):.1f}); tail {t:6.1f} ms (median of {n})")
    for p, pl in enumerate(plans):
        o, r = pl["owned"], pl["rects"][0]
        lines.append(f"    part {p} latent rows {o[0]}-{o[1]} cols {o[2]}-{o[3]}, video rows {r[0]}-{r[1]} cols {r[2]}-{r[3]}: {part_ms[p]:8.1f} ms")
    lines.append(f"    slowest part {slow:8.1f} ms + tail {t:.1f} ms   whole / (slowest part + tail) {w / (slow + t):.2f}x   "
                 f"(pixel counts alone, no tail: {shape[2] * shape[3] / crop:.2f}x)")
    lines.append("")
    print("\n".join(lines[-(n + 3):]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines))
print(f"wrote {out_path}")
