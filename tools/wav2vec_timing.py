"""Time the talk variant's audio encoder at the base size (chinese-wav2vec2-base: 512 / 768 / 3072, 12 heads, 12 blocks; random weights) for 10 s and 60 s
of audio: ms per svi_hip.WanAudioEncoder.encode on the device, beside the same call of the reference's class (utils/src/audio_analysis/wav2vec2.py through
get_embedding's arguments) on this box's CPU threads.  Either half is skipped, and the file says so, where this box lacks what it needs: a GPU, or the
reference tree (SVI_REFERENCE, default /root/reference) with transformers.  Reported, not gated.
    python tools/wav2vec_timing.py [--out profiles/wav2vec_timing.txt] [--seconds 10 60] [--cpu-repeats 1]
"""
import argparse
import os
import socket
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stable-video-infinity_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import wav2vec_cases as wc                                                                            # noqa: E402

BASE = dict(wc.BASE1, num_layers=12)
SEED = 4400


def device_ms(speech, repeats=5):
    import svi_hip
    sd = {k: torch.from_numpy(v) for k, v in wc.state_dict(SEED, BASE).items()}
    enc = svi_hip.WanAudioEncoder.from_state_dict(sd, wc.hf_config(BASE))
    out = {}
    for secs, x in speech.items():
        xd = torch.from_numpy(x).cuda()
        enc.encode(xd); torch.cuda.synchronize()                                                     # workspace allocation, LDS attributes
        t0 = time.perf_counter()
        for _ in range(repeats):
            y = enc.encode(xd)
        torch.cuda.synchronize()
        out[secs] = (time.perf_counter() - t0) / repeats * 1e3
        assert bool(torch.isfinite(y).all()) and tuple(y.shape) == (int(secs * 25), 12, 768)
    return out


def reference_ms(speech, repeats):
    ref = os.environ.get("SVI_REFERENCE", "/root/reference")
    if not os.path.isdir(os.path.join(ref, "utils", "src", "audio_analysis")):
        return None, f"no reference tree at {ref}"
    try:
        sys.path.insert(0, ref)
        from transformers import Wav2Vec2Config, Wav2Vec2FeatureExtractor
        from utils.src.audio_analysis.wav2vec2 import Wav2Vec2Model
    except ImportError as e:
        return None, f"reference class not importable: {e}"
    m = Wav2Vec2Model(Wav2Vec2Config(**wc.hf_config(BASE), attn_implementation="eager")).eval()
    parametrized = any("parametrizations" in k for k in m.state_dict())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in wc.state_dict(SEED, BASE, parametrized).items()}, strict=False)
    fx = Wav2Vec2FeatureExtractor(feature_size=1, sampling_rate=16000, padding_value=0.0, do_normalize=True, return_attention_mask=False)
    out = {}
    with torch.no_grad():
        for secs, x in speech.items():
            t0 = time.perf_counter()
            for _ in range(repeats):
                feat = torch.from_numpy(np.squeeze(fx(x, sampling_rate=16000).input_values)).float()[None]
                hs = m(feat, seq_len=int(len(x) / 16000 * 25), output_hidden_states=True).hidden_states
                y = torch.stack(hs[1:], dim=1)
            out[secs] = (time.perf_counter() - t0) / repeats * 1e3
            assert tuple(y.shape) == (1, 12, int(secs * 25), 768)
    return out, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wav2vec_timing.txt"))
    ap.add_argument("--seconds", type=float, nargs="+", default=[10, 60])
    ap.add_argument("--cpu-repeats", type=int, default=1)
    args = ap.parse_args()
    speech = {s: wc.waveform(50 + i, int(s * 16000)) for i, s in enumerate(args.seconds)}
    lines = [f"audio encoder, base size (12 blocks, fp32), random weights; host {socket.gethostname()}",
             "ms per encode of the whole waveform (normalisation, convolution stack, interpolation, 12 blocks, [N, 12, 768] written)"]
    if torch.cuda.is_available():
        d = device_ms(speech)
        lines.append(f"device: {torch.cuda.get_device_name(0)}")
        lines += [f"  {s:5.1f} s of audio ({int(s * 25):4d} frames): {ms:9.2f} ms on the device" for s, ms in d.items()]
    else:
        lines.append("device: no GPU on this box, not measured")
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    r, why = reference_ms(speech, args.cpu_repeats)
    if r is None:
        lines.append(f"reference class on the CPU: not measured ({why})")
    else:
        lines.append(f"reference class on the CPU, {torch.get_num_threads()} threads, fp32, eager attention, first call included ({args.cpu_repeats} call(s) averaged):")
        lines += [f"  {s:5.1f} s of audio ({int(s * 25):4d} frames): {ms:9.2f} ms on the CPU" for s, ms in r.items()]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
