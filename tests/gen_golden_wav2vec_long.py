"""Generate tests/golden/wav2vec_long.npz: the REFERENCE's audio encoder past 2048 frames, on seeded weights and waveforms.

The reference's own class on the CPU, in fp32 and in float64, exactly as tests/gen_golden_wav2vec.py runs it (reference_model, run_pair and hooked are that
file's, imported; nothing there changes).  Per tensor the fixture keeps the fp32 value, gap = max|fp32 - fp64| and rms, each over the KEPT rows: every 16th
row plus the last one (wav2vec_long_cases.kept_rows, coarser for the tensors of hundreds of thousands of rows) — the file stays under 1 MB.  The cases and
the tensors kept of each are wav2vec_long_cases'.  Neither weights nor waveforms are stored: wav2vec_cases.state_dict and wav2vec_cases.waveform rebuild
them from their seeds.  torch on the CPU only.

    python tests/gen_golden_wav2vec_long.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import wav2vec_cases as wc  # noqa: E402
from gen_golden import OUT, _reference_toplevel  # noqa: E402
from gen_golden_wav2vec import hooked, reference_model, run_pair  # noqa: E402,F401  (hooked: run_pair's own)
from wav2vec_long_cases import LONG_INPUTS, STAGES, kept_rows  # noqa: E402


def record(out: dict, prefix: str, f32: dict, f64: dict, names):
    for name in names:
        a, b = f32[name].float(), f64[name]
        assert a.dtype == torch.float32 and b.dtype == torch.float64 and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
        rows = torch.from_numpy(kept_rows(a.shape[0]))
        a, b = a[rows], b[rows]
        gap = float((a.double() - b).abs().max())
        rms = float(b.pow(2).mean().sqrt())
        out[f"{prefix}.{name}"] = a.numpy()
        out[f"{prefix}.{name}.gap"] = np.float64(gap)
        out[f"{prefix}.{name}.rms"] = np.float64(rms)
        print(f"  {prefix}.{name:8s} {tuple(a.shape)!s:16s} rms {rms:.4f}  gap {gap:.3e}", flush=True)


def main():
    torch.manual_seed(0)
    from einops import rearrange
    get_embedding = _reference_toplevel("utils/audio_process.py", "get_embedding", {"np": np, "torch": torch, "rearrange": rearrange})
    models, out = {}, {}
    for name, which, n, seed, S in LONG_INPUTS:
        cfg = dict(tiny=wc.TINY, base1=wc.BASE1)[which]
        if which not in models:
            models[which] = reference_model(cfg, wc.SEEDS[which])
        speech = wc.waveform(seed, n)
        f32, f64 = run_pair(models[which], speech, get_embedding, S)
        S = wc.seq_len(n) if S is None else S
        assert S > 2048 and tuple(f32["stack"].shape) == (S, cfg["num_layers"], cfg["hidden"]) and f32["conv6"].shape[0] == wc.frames(n)
        out[f"{name}.seq_len"], out[f"{name}.n_samples"], out[f"{name}.wave_seed"] = np.int64(S), np.int64(n), np.int64(seed)
        record(out, name, f32, f64, STAGES[name])
    path = os.path.join(OUT, "wav2vec_long.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"wrote {path} ({size} bytes)")
    assert size < 1000000, size


if __name__ == "__main__":
    main()
