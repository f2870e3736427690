"""Time the talk variant's audio encoder at the base size (chinese-wav2vec2-base: 512 / 768 / 3072, 12 heads, 12 blocks; random weights, as
tools/wav2vec_timing.py) on audio around and past the resident attention kernel's 2048 frames: by default 81 s (2025 frames, the resident kernel, a
handle left at its default limit), 84 s (2100 frames) and 600 s (15000 frames), the last two on a handle raised with max_frames.  Per length: one warm-up
encode (workspace allocation), then `--repeats` encodes timed one by one with device synchronisation; the median, the minimum and the maximum are written.
For the lengths past 2048 frames the streaming attention kernel is timed alone at the same shape (svi_hip.ops.encoder_attention, kernel 2, q | k | v side by
side as the encoder's blocks pass them), and 12 launches of it are set against the encode: its share.  Reported, not gated.
    python tools/wav2vec_long_timing.py [--out profiles/wav2vec_long_timing.txt] [--seconds 81 84 600] [--repeats 5]
A length that cannot be run (memory) is reported as such and the rest goes on.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if not os.environ.get("SVI_TIMING_PACKAGE"):                                                          # A/B: another checkout's package directory
    sys.path.insert(0, os.path.join(ROOT, "stable-video-infinity_amd"))
else:
    sys.path.insert(0, os.environ["SVI_TIMING_PACKAGE"])
sys.path.insert(0, os.path.join(ROOT, "tests"))
import wav2vec_cases as wc                                                                            # noqa: E402

BASE = dict(wc.BASE1, num_layers=12)
SEED = 4400


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wav2vec_long_timing.txt"))
    ap.add_argument("--seconds", type=float, nargs="+", default=[81, 84, 600])
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import svi_hip
    from svi_hip import ops
    assert torch.cuda.is_available(), "the timing needs a GPU"
    has_limit = hasattr(svi_hip.WanAudioEncoder, "max_frames")
    sd = {k: torch.from_numpy(v) for k, v in wc.state_dict(SEED, BASE).items()}
    lines = [f"audio encoder, base size (12 blocks of 12 heads of 64, fp32), random weights; {torch.cuda.get_device_name(0)}; package {os.path.dirname(svi_hip.__file__)}",
             f"ms per encode of the whole waveform, one warm-up encode, then {args.repeats} encodes timed one by one: median (min .. max)"]
    for i, secs in enumerate(args.seconds):
        S = int(secs * 25)
        if S > 2048 and not has_limit:
            lines.append(f"  {secs:6.1f} s of audio ({S:5d} frames): not served by this package (no max_frames)")
            continue
        try:
            enc = svi_hip.WanAudioEncoder.from_state_dict(sd, wc.hf_config(BASE), **(dict(max_frames=S) if S > 2048 else {}))
            x = torch.from_numpy(wc.waveform(50 + i, int(secs * 16000))).cuda()
            med, lo, hi = timed(lambda: enc.encode(x), args.repeats)
            y = enc.encode(x)
            assert tuple(y.shape) == (S, 12, 768) and bool(torch.isfinite(y).all())
            line = f"  {secs:6.1f} s of audio ({S:5d} frames): {med:10.2f} ms ({lo:.2f} .. {hi:.2f}), attention: {'resident' if S <= 2048 else 'streaming'} kernel"
            del y
            if S > 2048:
                qkv = torch.randn(S, 3 * 768, device="cuda")
                q, k, v = (qkv[:, j * 768:(j + 1) * 768].unflatten(1, (12, 64)) for j in range(3))
                out = torch.empty(S, 12, 64, device="cuda")
                a_med, a_lo, a_hi = timed(lambda: ops.encoder_attention(q, k, v, kernel=2, out=out), args.repeats)
                flop = 4.0 * S * S * 64 * 12
                line += (f"; one launch of it alone {a_med:.2f} ms ({a_lo:.2f} .. {a_hi:.2f}) = {flop / a_med / 1e9:.1f} TFLOP/s fp32; "
                         f"12 launches = {12 * a_med:.1f} ms = {100 * 12 * a_med / med:.0f} % of the encode")
                del qkv, out
            lines.append(line)
            del enc, x
            torch.cuda.empty_cache()
        except RuntimeError as e:                                                                      # out of memory on this box: say so, go on
            if "out of memory" not in str(e).lower() and "hipMalloc" not in str(e):
                raise                                                                                  # anything else ends the run
            lines.append(f"  {secs:6.1f} s of audio ({S:5d} frames): not run ({str(e).splitlines()[0][:160]})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
