"""Shared by tests/gen_golden_wav2vec.py, tests/test_wav2vec_host.py, tests/test_gpu_wav2vec.py and examples/svi_talk_audio_hip.py --synthetic: the audio
encoder's test configurations, the formula that rebuilds their weights from a seed (the fixtures store no weights), seeded waveforms, and the parity bound.

Weights: every tensor is drawn from its own RandomState(seed + index in the sorted key list); matrices and convolutions are scaled by 1 / sqrt(fan_in) so that
activations stay of order one through the stack, norm gains are 1 + 0.1 n, biases 0.1 n.  The positional convolution comes as weight norm's pair (g, v) under
either spelling of its keys."""
from __future__ import annotations

import numpy as np

CONV_KERNEL, CONV_STRIDE = (10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2)

# constructor arguments of svi_hip.WanAudioEncoder
TINY = dict(conv_dim=32, hidden=128, ffn=256, num_heads=2, num_layers=2, pos_kernel=128, pos_groups=16, eps=1e-5)
BASE1 = dict(conv_dim=512, hidden=768, ffn=3072, num_heads=12, num_layers=1, pos_kernel=128, pos_groups=16, eps=1e-5)
# what the talk DiT reads ([N, 12, 768]) on a small convolution stack and feed-forward: the talk stream's tests and the example's --synthetic
TALK_TINY = dict(conv_dim=32, hidden=768, ffn=128, num_heads=12, num_layers=12, pos_kernel=128, pos_groups=16, eps=1e-5)
SEEDS = dict(tiny=4100, base1=4200, talk_tiny=4300)

# fixture inputs: (name, samples, waveform seed, seq_len or None = get_embedding's int(seconds * 25)).  0.6 s -> seq_len 15 (29 frames interpolated down);
# 0.25 s -> seq_len 6 from 12 frames; the same 0.25 s asked for 20 frames: the interpolation upsamples (the reference class takes seq_len as an argument;
# get_embedding's own rule always halves).  The positional convolution's padding (64) exceeds the sequence in all three.
# d, e: odd sample counts whose last window is ragged at several layers (5123 = 16 * 320 + 3, 6077 = 18 * 320 + 317); f: 700 samples are ONE frame and seq_len 1.
TINY_INPUTS = (("a", 9600, 11, None), ("b", 4000, 12, None), ("c", 4000, 12, 20), ("d", 5123, 14, None), ("e", 6077, 15, None), ("f", 700, 16, None))
BASE1_INPUT = ("a", 16000, 13, None)
BASE1_ROWS = slice(0, None, 4)              # rows of the last convolution layer's output the base-width fixture keeps

PG, PV = "encoder.pos_conv_embed.conv.weight_g", "encoder.pos_conv_embed.conv.weight_v"
PG_P, PV_P = "encoder.pos_conv_embed.conv.parametrizations.weight.original0", "encoder.pos_conv_embed.conv.parametrizations.weight.original1"


def hf_config(cfg: dict) -> dict:
    """The Wav2Vec2Config arguments (= config.json) of a configuration."""
    return dict(hidden_size=cfg["hidden"], intermediate_size=cfg["ffn"], num_attention_heads=cfg["num_heads"], num_hidden_layers=cfg["num_layers"],
                conv_dim=[cfg["conv_dim"]] * 7, conv_kernel=list(CONV_KERNEL), conv_stride=list(CONV_STRIDE), conv_bias=False, feat_extract_norm="group",
                feat_extract_activation="gelu", hidden_act="gelu", num_conv_pos_embeddings=cfg["pos_kernel"], num_conv_pos_embedding_groups=cfg["pos_groups"],
                layer_norm_eps=cfg["eps"], do_stable_layer_norm=False, add_adapter=False, vocab_size=32, hidden_dropout=0.0, activation_dropout=0.0,
                attention_dropout=0.0, feat_proj_dropout=0.0, final_dropout=0.0, layerdrop=0.0, mask_time_prob=0.0, mask_feature_prob=0.0)


def shapes(cfg: dict, parametrized: bool = False) -> dict:
    C, H, F = cfg["conv_dim"], cfg["hidden"], cfg["ffn"]
    s = {}
    for i, k in enumerate(CONV_KERNEL):
        s[f"feature_extractor.conv_layers.{i}.conv.weight"] = (C, 1 if i == 0 else C, k)
    s["feature_extractor.conv_layers.0.layer_norm.weight"] = s["feature_extractor.conv_layers.0.layer_norm.bias"] = (C,)
    s["feature_projection.layer_norm.weight"] = s["feature_projection.layer_norm.bias"] = (C,)
    s["feature_projection.projection.weight"], s["feature_projection.projection.bias"] = (H, C), (H,)
    s[PG_P if parametrized else PG] = (1, 1, cfg["pos_kernel"])
    s[PV_P if parametrized else PV] = (H, H // cfg["pos_groups"], cfg["pos_kernel"])
    s["encoder.pos_conv_embed.conv.bias"] = (H,)
    s["encoder.layer_norm.weight"] = s["encoder.layer_norm.bias"] = (H,)
    for i in range(cfg["num_layers"]):
        b = f"encoder.layers.{i}."
        for p in ("q_proj", "k_proj", "v_proj", "out_proj"):
            s[b + f"attention.{p}.weight"], s[b + f"attention.{p}.bias"] = (H, H), (H,)
        s[b + "layer_norm.weight"] = s[b + "layer_norm.bias"] = s[b + "final_layer_norm.weight"] = s[b + "final_layer_norm.bias"] = (H,)
        s[b + "feed_forward.intermediate_dense.weight"], s[b + "feed_forward.intermediate_dense.bias"] = (F, H), (F,)
        s[b + "feed_forward.output_dense.weight"], s[b + "feed_forward.output_dense.bias"] = (H, F), (H,)
    return s


def state_dict(seed: int, cfg: dict, parametrized: bool = False) -> dict:
    """fp32 numpy state dict of a Wav2Vec2Model of this configuration; the same values under either spelling of the weight-norm keys."""
    plain = shapes(cfg, False)
    out = {}
    for idx, key in enumerate(sorted(plain)):
        shape = plain[key]
        n = np.random.RandomState(seed + idx).standard_normal(shape).astype(np.float32)
        if key == PG:
            v = 1.0 + 0.1 * np.abs(n)
        elif key.endswith("layer_norm.weight"):
            v = 1.0 + 0.1 * n
        elif key.endswith(".bias"):
            v = 0.1 * n
        else:
            fan_in = int(np.prod(shape[1:]))
            v = n * np.float32(1.5 / np.sqrt(fan_in))
        name = {PG: PG_P, PV: PV_P}.get(key, key) if parametrized else key
        out[name] = np.ascontiguousarray(v, dtype=np.float32)
    return out


def waveform(seed: int, n: int) -> np.ndarray:
    """A voiced-looking test signal at 16 kHz: a few harmonics under a slow envelope plus noise, peak about 0.3, fp32."""
    r = np.random.RandomState(seed)
    t = np.arange(n, dtype=np.float64) / 16000.0
    f0 = 110.0 + 40.0 * r.rand()
    x = sum(a * np.sin(2 * np.pi * f0 * (h + 1) * t + 2 * np.pi * r.rand()) for h, a in enumerate((0.5, 0.3, 0.2, 0.1)))
    x = x * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t)) * 0.25 + 0.02 * r.standard_normal(n) + 0.01
    return x.astype(np.float32)


def frames(n: int, upto: int = 7) -> int:
    for k, s in list(zip(CONV_KERNEL, CONV_STRIDE))[:upto]:
        n = (n - k) // s + 1 if n >= k else 0
    return n


def seq_len(n: int) -> int:
    return int(n / 16000 * 25)


def bound(gap: float, rms: float) -> float:
    """max|device - reference fp32| allowed for one tensor: four times the reference's own distance from its float64 twin (another summation order than the
    reference's fp32 run) plus 1e-6 of the tensor's rms."""
    return 4.0 * float(gap) + 1e-6 * float(rms)
