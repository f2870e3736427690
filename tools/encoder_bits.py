"""One sha256 per device result of the three once-per-clip encoders on their tiny test configurations (fixed seeds): the text encoder's and the image
encoder's forwards, the audio encoder's forward and every svi_w2v_forward_stage stage, and svi_encoder_attention_f32 under kernels 0 / 1 / 2 at 2048 and
2049 keys (both sides of the resident / streaming boundary) for two head sizes.  Run it on two builds (SVI_HIP_LIB selects the library) and compare
the tables: a restructuring of the encoders' host code or a move of their kernels must leave every line as it was.
    python tools/encoder_bits.py [--out FILE]
"""
import argparse
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stable-video-infinity_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import synth                                                                                         # noqa: E402
import wav2vec_cases as wc                                                                            # noqa: E402


def digest(t: torch.Tensor) -> str:
    torch.cuda.synchronize()
    t = t.detach().contiguous().cpu()
    raw = (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy().tobytes()
    return hashlib.sha256(raw).hexdigest()[:32]


def rows():
    import svi_hip
    from svi_hip import ops
    dev = "cuda"
    te = svi_hip.WanTextEncoder.from_state_dict({k: torch.from_numpy(v) for k, v in synth.t5_state_dict(synth.T5_SEED, **synth.T5_TINY).items()})
    for name, Ln, valid, seed in synth.T5_TINY_CASES:
        ids, mask = synth.t5_ids(seed, Ln, valid, synth.T5_TINY["vocab"])
        for mode in ("all", "valid"):
            yield f"t5 {name} rows={mode}", te.forward(torch.from_numpy(ids), torch.from_numpy(mask), rows=mode)
    ie = svi_hip.WanImageEncoder.from_state_dict({k: torch.from_numpy(v) for k, v in synth.clip_state_dict(synth.CLIP_SEED, **synth.CLIP_TINY).items()},
                                                 num_heads=synth.CLIP_TINY["num_heads"])
    for name, shape, seed in synth.CLIP_TINY_CASES:
        yield f"clip {name}", ie.encode_image([torch.from_numpy(synth.clip_image(seed, *shape))])
    ae = svi_hip.WanAudioEncoder.from_state_dict({k: torch.from_numpy(v) for k, v in wc.state_dict(wc.SEEDS["tiny"], wc.TINY).items()}, wc.hf_config(wc.TINY))
    stages = ["wave"] + [("conv", i) for i in range(7)] + ["interp", "proj", "pos", "enc_ln"] + [("layer", i) for i in range(wc.TINY["num_layers"])]
    for name, n, seed, S in wc.TINY_INPUTS:
        x = wc.waveform(seed, n)
        yield f"w2v {name} forward f32", ae.encode(x, seq_len=S)
        yield f"w2v {name} forward bf16", ae.encode(x, seq_len=S, dtype=torch.bfloat16)
        for st in stages:
            yield f"w2v {name} stage {st}", ae.stage(x, st, seq_len=S)
    g = torch.Generator(device=dev).manual_seed(77)
    for heads, D in ((2, 64), (1, 80)):
        for Lk in (2048, 2049):
            q = torch.randn(19, heads, D, device=dev, generator=g)
            k = torch.randn(Lk, heads, D, device=dev, generator=g)
            v = torch.randn(Lk, heads, D, device=dev, generator=g)
            for kernel in (0, 1, 2):
                tag = f"attention D={D} heads={heads} Lq=19 Lk={Lk} kernel={kernel}"
                if kernel == 1 and Lk > ops.ENCODER_ATTENTION_RESIDENT_KEYS:
                    try:
                        ops.encoder_attention(q, k, v, kernel=kernel)
                        yield tag, None, "ACCEPTED (the resident kernel must refuse this)"
                    except RuntimeError:
                        yield tag, None, "refused"
                else:
                    yield tag, ops.encoder_attention(q, k, v, kernel=kernel)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for row in rows():
        name, t = row[0], row[1]
        lines.append(f"{name:52s} {digest(t) if t is not None else row[2]}")
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
