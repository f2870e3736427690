"""Time the LoRA merge into FP8-stored weights for the 14B-I2V target set against the reference's own arithmetic in PyTorch on the same device.

Target set: 40 blocks x (self-attention q / k / v / o, cross-attention q / k / v / o at 5120 x 5120, ffn.0 at 13824 x 5120, ffn.2 at 5120 x 13824),
rank 128, synthetic data.  One block's ten matrices are resident (351 MB of e4m3 codes — more than the Infinity Cache holds, so every pass streams
them from HBM) and walked 40 times per measurement.  Three things are timed, alternating, after a warm-up pass of each:
    hip      lora.merge_lora_ as a user calls it (the transpose of `down` included)
    kernel   svi_lora_merge_e4m3 alone on prepared operands
    torch    w8.copy_((w8.float() + alpha * torch.mm(up.float(), down.float())).to(torch.float8_e4m3fn)) — dequantise, fp32 mm, add, cast
The W8 stream is 2 bytes per element (read once, written once); its rate is reported for each.

    python tools/lora_merge_time.py [--operands bf16|f32] [--rounds 3] [--blocks 40] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stable-video-infinity_amd"))

import torch  # noqa: E402

DIM, FFN, RANK = 5120, 13824, 128
SHAPES = [(DIM, DIM)] * 8 + [(FFN, DIM), (DIM, FFN)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--operands", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=40)
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "timing needs the GPU"
    from svi_hip import _lib as L
    from svi_hip import lora
    dev = torch.device("cuda", 0)
    dt = torch.bfloat16 if args.operands == "bf16" else torch.float32
    g = torch.Generator(device=dev).manual_seed(0)
    mats = []
    for out_f, in_f in SHAPES:
        w8 = (0.05 * torch.randn((out_f, in_f), generator=g, device=dev)).to(torch.float8_e4m3fn)
        # small operands: 400 merges in a row must not walk the synthetic weights out of e4m3's range
        up = (0.003 * torch.randn((out_f, RANK), generator=g, device=dev)).to(dt)
        down = (0.003 * torch.randn((RANK, in_f), generator=g, device=dev)).to(dt)
        mats.append((w8, up, down, down.t().contiguous()))
    stream_bytes = 2 * sum(o * i for o, i in SHAPES) * args.blocks
    code = {torch.bfloat16: L.SVI_BF16, torch.float32: L.SVI_F32}[dt]

    def run_hip():
        for w8, up, down, _ in mats:
            lora.merge_lora_(w8, up, down, args.alpha)

    def run_kernel():
        lib, st = L.lib(), L.current_stream()
        for w8, up, _, down_t in mats:
            L.check(lib.svi_lora_merge_e4m3(L.ptr(w8), w8.shape[0], w8.shape[1], L.ptr(up), L.ptr(down_t), code, RANK, args.alpha, st), "merge")

    def run_torch():
        for w8, up, down, _ in mats:
            w8.copy_((w8.float() + args.alpha * torch.mm(up.float(), down.float())).to(torch.float8_e4m3fn))

    runs = {"hip": run_hip, "kernel": run_kernel, "torch": run_torch}

    def timed(fn) -> float:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.blocks):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    for fn in runs.values():          # warm-up: code objects, allocator, BLAS algorithm choice
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            ms[k].append(timed(fn))
    rec = {"lora_merge_time": {"model": "14b-i2v", "blocks": args.blocks, "merges": args.blocks * len(SHAPES), "rank": RANK, "operands": args.operands,
                               "w8_stream_bytes": stream_bytes,
                               **{k: {"ms_rounds": [round(v, 3) for v in vs], "ms_median": round(statistics.median(vs), 3),
                                      "w8_stream_TB_per_s": round(stream_bytes / (statistics.median(vs) * 1e-3) / 1e12, 3)} for k, vs in ms.items()}}}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main()
