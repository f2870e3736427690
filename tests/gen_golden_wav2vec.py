"""Generate tests/golden/wav2vec_tiny.npz and tests/golden/wav2vec_base1.npz: the REFERENCE's audio encoder on seeded weights and waveforms.

Nothing of the reference is restated here.  The model is the reference's own class (utils/src/audio_analysis/wav2vec2.py Wav2Vec2Model, imported where it
lies), the call is the reference's own get_embedding compiled out of utils/audio_process.py (gen_golden._reference_toplevel: executed, not copied; the
module's other imports — pyloudnorm, librosa — are not needed) with transformers' Wav2Vec2FeatureExtractor, as test_svi_talk.py sets it up.  Intermediates
are read with forward hooks.  The same model runs once more in float64 (the feature extractor's own normalisation on the float64 samples, the model cast
with .double()); per tensor the fixture keeps the fp32 value, gap = max|fp32 - fp64| and rms — the parity bound of tests/test_gpu_wav2vec.py is made of
those two (wav2vec_cases.bound).  Weights are not stored: wav2vec_cases.state_dict rebuilds them from the seed.  torch on the CPU only.

    python tests/gen_golden_wav2vec.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import wav2vec_cases as wc  # noqa: E402
from gen_golden import OUT, REF, _reference_toplevel  # noqa: E402


def reference_model(cfg: dict, seed: int):
    sys.path.insert(0, REF)
    from transformers import Wav2Vec2Config
    from utils.src.audio_analysis.wav2vec2 import Wav2Vec2Model
    # eager attention: what the reference's transformers ran, and the only implementation its forward's `config.output_attentions = True` allows today
    m = Wav2Vec2Model(Wav2Vec2Config(**wc.hf_config(cfg), attn_implementation="eager")).eval()
    parametrized = any("parametrizations" in k for k in m.state_dict())
    sd = {k: torch.from_numpy(v) for k, v in wc.state_dict(seed, cfg, parametrized).items()}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and set(missing) <= {"masked_spec_embed"}, (missing, unexpected)
    return m


def hooked(model, run):
    """run() with forward hooks on every stage -> {name: tensor [rows, channels]}."""
    got, hooks = {}, []

    def keep(name, pick):
        def hook(_mod, args, out):
            got[name] = pick(args, out).detach().clone()
        return hook
    fe = model.feature_extractor
    for i, layer in enumerate(fe.conv_layers):
        hooks.append(layer.register_forward_hook(keep(f"conv{i}", lambda a, o: o[0].transpose(0, 1))))
    hooks.append(fe.register_forward_hook(keep("wave", lambda a, o: a[0][0])))
    hooks.append(model.feature_projection.register_forward_hook(keep("interp", lambda a, o: a[0][0])))
    hooks.append(model.feature_projection.register_forward_hook(keep("proj", lambda a, o: o[0][0])))
    hooks.append(model.encoder.pos_conv_embed.register_forward_hook(keep("pos", lambda a, o: o[0])))
    hooks.append(model.encoder.layer_norm.register_forward_hook(keep("enc_ln", lambda a, o: o[0])))
    for i, layer in enumerate(model.encoder.layers):
        hooks.append(layer.register_forward_hook(keep(f"layer{i}", lambda a, o: (o[0] if isinstance(o, tuple) else o)[0])))
    try:
        got["stack"] = run()
    finally:
        for h in hooks:
            h.remove()
    return got


def run_pair(model, speech: np.ndarray, get_embedding, seq_len=None):
    """({name: fp32 tensor}, {name: float64 tensor}) of one waveform; seq_len=None: through get_embedding, else the model called with that seq_len on the
    feature extractor's output, stacked as get_embedding stacks."""
    from transformers import Wav2Vec2FeatureExtractor
    fx = Wav2Vec2FeatureExtractor(feature_size=1, sampling_rate=16000, padding_value=0.0, do_normalize=True, return_attention_mask=False)
    with torch.no_grad():
        S = wc.seq_len(len(speech)) if seq_len is None else seq_len

        def stacked(m, wave):
            hs = m(wave, seq_len=S, output_hidden_states=True).hidden_states
            return torch.stack(hs[1:], dim=1).squeeze(0).transpose(0, 1)
        if seq_len is None:
            f32 = hooked(model, lambda: get_embedding(speech, fx, model, sr=16000, device="cpu"))
        else:
            wave32 = torch.from_numpy(np.squeeze(fx(speech, sampling_rate=16000).input_values)).float()[None]
            f32 = hooked(model, lambda: stacked(model, wave32))
        m64 = model.double()
        wave64 = torch.from_numpy(fx.zero_mean_unit_var_norm([speech.astype(np.float64)], attention_mask=None)[0])[None]
        assert wave64.dtype == torch.float64
        f64 = hooked(m64, lambda: stacked(m64, wave64))
        model.float()
    return f32, f64


def record(out: dict, prefix: str, f32: dict, f64: dict, names, rows=None):
    for name in names:
        a, b = f32[name].float(), f64[name]
        assert a.dtype == torch.float32 and b.dtype == torch.float64 and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
        if rows is not None and name in rows:
            a, b = a[rows[name]], b[rows[name]]
        gap = float((a.double() - b).abs().max())
        rms = float(b.pow(2).mean().sqrt())
        out[f"{prefix}.{name}"] = a.numpy()
        out[f"{prefix}.{name}.gap"] = np.float64(gap)
        out[f"{prefix}.{name}.rms"] = np.float64(rms)
        print(f"  {prefix}.{name:8s} {tuple(a.shape)!s:16s} rms {rms:.4f}  gap {gap:.3e}")


def main():
    torch.manual_seed(0)
    from einops import rearrange
    get_embedding = _reference_toplevel("utils/audio_process.py", "get_embedding", {"np": np, "torch": torch, "rearrange": rearrange})
    # ---- tiny: every intermediate of input a, everything after the convolution stack of input b
    model = reference_model(wc.TINY, wc.SEEDS["tiny"])
    out = {}
    stages = ["wave"] + [f"conv{i}" for i in range(7)] + ["interp", "proj", "pos", "enc_ln"] + [f"layer{i}" for i in range(wc.TINY["num_layers"])] + ["stack"]
    for name, n, seed, S in wc.TINY_INPUTS:
        speech = wc.waveform(seed, n)
        f32, f64 = run_pair(model, speech, get_embedding, S)
        S = wc.seq_len(n) if S is None else S
        assert tuple(f32["stack"].shape) == (S, wc.TINY["num_layers"], wc.TINY["hidden"]) and f32["conv6"].shape[0] == wc.frames(n)
        out[f"{name}.samples"], out[f"{name}.seq_len"] = speech, np.int64(S)
        record(out, name, f32, f64, stages if name == "a" else [s for s in stages if not s.startswith("conv")] + ["conv6"])
    path = os.path.join(OUT, "wav2vec_tiny.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    # ---- base widths, one block: the final stack and a sample of the convolution stack's rows
    model = reference_model(wc.BASE1, wc.SEEDS["base1"])
    name, n, seed, _ = wc.BASE1_INPUT
    speech = wc.waveform(seed, n)
    f32, f64 = run_pair(model, speech, get_embedding)
    out = {f"{name}.samples": speech, f"{name}.seq_len": np.int64(wc.seq_len(n))}
    record(out, name, f32, f64, ["conv6", "stack"], rows={"conv6": wc.BASE1_ROWS})
    path = os.path.join(OUT, "wav2vec_base1.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
