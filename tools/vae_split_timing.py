"""One rank's part of the exact VAE decode split next to the whole decode, on ONE GPU: the whole decode at [16, 21, 60, 104] alternated with each part
of a 1x2, 2x2 and 2x4 split (WanVideoVAE.decode_part into a tight buffer, as a rank of the latency modes would run it).  Every timing sits between HIP
events after a warm-up of the same call.  These are per-part times of one device, not a scaling run: no all-gather, no second GPU.
    python tools/vae_split_timing.py [--out profiles/vae_split_timing.txt] [--small]
Reports ms for the whole decode, ms per part, the slowest part and whole / slowest part, next to DESIGN §5's projection (which assumed the first halo is
carried through all four stages; the planner trims it per stage)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stable-video-infinity_amd"))
import torch
from svi_hip import _lib
from svi_hip.vae import WanVideoVAE, device_vae_weights

args = sys.argv[1:]
out_path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "vae_split_timing.txt")
shape = (16, 3, 32, 40) if "--small" in args else (16, 21, 60, 104)
PROJECTION = {(1, 2): 1.58, (2, 2): 2.15, (2, 4): 2.6}

dev = torch.device("cuda")
vae = WanVideoVAE.from_state_dict(device_vae_weights(0, dev))
z = torch.randn(shape, generator=torch.Generator(device=dev).manual_seed(3), device=dev)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); out = fn(); e1.record(); torch.cuda.synchronize()
    del out
    return e0.elapsed_time(e1)


whole = lambda: vae.decode([z], device=dev)      # noqa: E731
timed(whole)                                     # warm-up: pool, LDS attributes, weight packing
lines = [f"VAE decode split timing, latent {list(shape)}, one GPU ({torch.cuda.get_device_name(0)}): per-part times, not a scaling run", ""]
for split in ((1, 2), (2, 2), (2, 4)):
    n = split[0] * split[1]
    whole_ms, part_ms = [], []
    for p in range(n):
        part = lambda p=p: vae.decode_part(z, split, p)      # noqa: E731
        timed(part)                              # warm-up of this part's shapes
        whole_ms.append(timed(whole))
        part_ms.append(timed(part))
    w = sorted(whole_ms)[len(whole_ms) // 2]
    slow = max(part_ms)
    owned = [_lib.vae_split_plan(shape[2], shape[3], *split, p)["owned"] for p in range(n)]
    lines.append(f"split {split[0]}x{split[1]}: whole {w:8.1f} ms (median of {n}, min {min(whole_ms):.1f} max {max(whole_ms):.1f})")
    for p in range(n):
        lines.append(f"    part {p} latent rows {owned[p][0]}-{owned[p][1]} cols {owned[p][2]}-{owned[p][3]}: {part_ms[p]:8.1f} ms")
    lines.append(f"    slowest part {slow:8.1f} ms   whole / slowest part {w / slow:.2f}x   (DESIGN §5 projection, halo carried through: {PROJECTION[split]:.2f}x)")
    lines.append("")
    print("\n".join(lines[-(n + 3):]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines))
print(f"wrote {out_path}")
