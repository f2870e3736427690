"""The audio encoder's boundary without a GPU: the C ABI's new symbols, the frame count of the convolution stack, every refusal of svi_w2v_create and
svi_w2v_forward (they come before anything touches the device), the weight-norm folding, and the checkpoint-directory loader's parsing (its binding needs a
device: the loader is driven up to the state dict it would bind)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import wav2vec_cases as wc
from svi_hip import _lib as L

NEW = ("svi_w2v_create", "svi_w2v_destroy", "svi_w2v_bind_weight", "svi_w2v_check_bound", "svi_w2v_frames", "svi_w2v_forward", "svi_w2v_forward_stage")


def _handle(cfg=wc.TINY):
    h = C.c_void_p()
    c = L.W2vConfig(cfg["conv_dim"], cfg["hidden"], cfg["ffn"], cfg["num_heads"], cfg["num_layers"], cfg["pos_kernel"], cfg["pos_groups"], cfg["eps"])
    status = L.lib().svi_w2v_create(C.byref(c), C.byref(h))
    return status, h


def _bind_everything(h, cfg=wc.TINY, skip=()):
    """Every key of the folded state dict at a made-up, aligned address: binding records pointers, it does not read them."""
    sh = wc.shapes(cfg)
    sh["encoder.pos_conv_embed.conv.weight"] = sh.pop(wc.PV)
    sh.pop(wc.PG)
    for name, shape in sh.items():
        if name in skip:
            continue
        arr = (C.c_int64 * len(shape))(*shape)
        assert L.lib().svi_w2v_bind_weight(h, name.encode(), 4096, L.SVI_F32, arr, len(shape)) == 0, (name, L.last_error())


def test_new_symbols_are_declared_exported_and_typed():
    from test_abi import declared_symbols
    table = {n: (r, a) for n, r, a in L.SYMBOLS}
    lib = L.lib()
    for n in NEW:
        assert n in declared_symbols() and n in table and hasattr(lib, n), n
        assert table[n][0] is C.c_int32
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert table["svi_w2v_bind_weight"][1] == table["svi_t5_bind_weight"][1] == table["svi_clip_bind_weight"][1]
    assert table["svi_w2v_frames"][1][0] is i64
    assert table["svi_w2v_forward"][1] == [vp, vp, i64, i32, vp, i32, vp]
    assert [f for f, _ in L.W2vConfig._fields_] == ["conv_dim", "hidden", "ffn", "num_heads", "num_layers", "pos_kernel", "pos_groups", "eps"]


def test_frames_is_the_reference_conv_length_formula():
    """Wav2Vec2PreTrainedModel._get_feat_extract_output_lengths: floor((n - k) / s) + 1 per layer — transformers' own method where it can be imported, and the helper's,
    on 400 .. 48000 samples in steps that visit every residue mod 320 (the stack's total stride) many times, and every count around each multiple."""
    try:
        from transformers import Wav2Vec2Config, Wav2Vec2Model
        ref = Wav2Vec2Model(Wav2Vec2Config(**wc.hf_config(wc.TINY)))._get_feat_extract_output_lengths
    except Exception:                       # not installed, or not importable in this process (other tests leave stand-in modules in sys.modules)
        ref = wc.frames
    from svi_hip.encoders import audio_frames
    counts = sorted(set(range(400, 48001, 7)) | set(range(400, 400 + 3 * 320)) | {48000} | {m * 320 + d for m in range(2, 150) for d in (-1, 0, 1, 79, 80, 81)})
    assert {n % 320 for n in counts} == set(range(320))
    for n in counts:
        assert audio_frames(n) == int(ref(n)) == wc.frames(n), n
    assert audio_frames(400) == 1 and audio_frames(399) == 0 and audio_frames(0) == 0 and audio_frames(16000) == 49


def test_create_refuses_a_head_size_the_attention_kernel_lacks():
    status, _ = _handle(dict(wc.TINY, hidden=96, num_heads=2))               # 48
    assert status != 0 and "head dim 48" in L.last_error()
    status, _ = _handle(dict(wc.TINY, hidden=128, num_heads=3))
    assert status != 0
    status, h = _handle()
    assert status == 0
    assert L.lib().svi_w2v_destroy(h) == 0


def test_bind_rejects_unknown_names_shapes_and_dtypes():
    lib = L.lib()
    _, h = _handle()
    ok = (C.c_int64 * 3)(128, 8, 128)
    assert lib.svi_w2v_bind_weight(h, b"encoder.pos_conv_embed.conv.weight", 4096, L.SVI_F32, ok, 3) == 0
    assert lib.svi_w2v_bind_weight(h, b"encoder.pos_conv_embed.conv.weight_v", 4096, L.SVI_F32, ok, 3) != 0 and "unknown" in L.last_error()
    bad = (C.c_int64 * 3)(128, 128, 128)
    assert lib.svi_w2v_bind_weight(h, b"encoder.pos_conv_embed.conv.weight", 4096, L.SVI_F32, bad, 3) != 0 and "shape mismatch" in L.last_error()
    assert lib.svi_w2v_bind_weight(h, b"encoder.pos_conv_embed.conv.weight", 4096, L.SVI_BF16, ok, 3) != 0 and "fp32" in L.last_error()
    assert lib.svi_w2v_bind_weight(h, b"encoder.pos_conv_embed.conv.weight", 4100, L.SVI_F32, ok, 3) != 0 and "aligned" in L.last_error()
    one = (C.c_int64 * 1)(128)
    assert lib.svi_w2v_bind_weight(h, b"masked_spec_embed", 4096, L.SVI_F32, one, 1) == 0         # accepted and ignored
    assert lib.svi_w2v_bind_weight(h, b"encoder.layers.2.layer_norm.weight", 4096, L.SVI_F32, one, 1) != 0   # two layers: 0 and 1
    lib.svi_w2v_destroy(h)


def test_forward_refusals_come_with_their_messages_before_the_device():
    lib = L.lib()
    _, h = _handle()
    fwd = lambda n, S, dtype=L.SVI_F32: lib.svi_w2v_forward(h, 4096, n, S, 8192, dtype, None)      # noqa: E731
    # nothing bound
    assert lib.svi_w2v_check_bound(h) == 2 and "never bound" in L.last_error()
    assert fwd(9600, 15) == 2 and "never bound" in L.last_error()
    missing = "encoder.layers.1.feed_forward.output_dense.bias"
    _bind_everything(h, skip=(missing,))
    assert fwd(9600, 15) == 2 and missing in L.last_error()
    _bind_everything(h)
    assert lib.svi_w2v_check_bound(h) == 0
    # more frames than the encoder attention has keys
    assert fwd(16000 * 90, 2049) != 0
    assert "2048" in L.last_error() and "81 s" in L.last_error()
    # fewer than one frame, fewer than one sample, shorter than the receptive field
    assert fwd(9600, 0) != 0 and "seq_len 0" in L.last_error()
    assert fwd(9600, -3) != 0 and "seq_len -3" in L.last_error()
    assert fwd(0, 15) != 0 and "0 samples" in L.last_error()
    assert fwd(-5, 15) != 0 and "-5 samples" in L.last_error()
    assert fwd(399, 1) != 0 and "400 samples" in L.last_error()
    # an output type the writer does not have
    assert fwd(9600, 15, L.SVI_F16) != 0 and "fp32 or bf16" in L.last_error()
    # the stage entry point refuses alike, and a stage that does not exist
    assert lib.svi_w2v_forward_stage(h, 4096, 9600, 2049, 0, 8192, 10, None) != 0 and "2048" in L.last_error()
    assert lib.svi_w2v_forward_stage(h, 4096, 9600, 15, 14, 8192, 10, None) != 0 and "no stage 14" in L.last_error()
    lib.svi_w2v_destroy(h)


@pytest.mark.parametrize("parametrized", [False, True], ids=["weight_g_v", "parametrizations"])
def test_weight_norm_folding_is_torch_weight_norm(parametrized):
    from svi_hip.encoders import fold_weight_norm
    sd = {k: torch.from_numpy(v) for k, v in wc.state_dict(wc.SEEDS["tiny"], wc.TINY, parametrized).items()}
    g, v = (sd[wc.PG_P], sd[wc.PV_P]) if parametrized else (sd[wc.PG], sd[wc.PV])
    want = torch._weight_norm(v, g, 2)
    got = fold_weight_norm(sd)
    assert not any("weight_g" in k or "weight_v" in k or "parametrizations" in k for k in got)
    w = got["encoder.pos_conv_embed.conv.weight"]
    assert w.dtype == torch.float32 and tuple(w.shape) == tuple(v.shape)
    # one division and one multiplication per element in another order than torch's kernel: a few ulp
    assert float((w - want).abs().max()) <= 4 * float(np.finfo(np.float32).eps) * float(want.abs().max())
    assert set(got) - {"encoder.pos_conv_embed.conv.weight"} == set(sd) - {wc.PG, wc.PV, wc.PG_P, wc.PV_P}
    assert fold_weight_norm(got).keys() == got.keys()                                  # already plain: unchanged
    with pytest.raises(KeyError):
        fold_weight_norm({k: t for k, t in sd.items() if k not in (wc.PG, wc.PG_P)})


@pytest.mark.parametrize("fmt", ["safetensors", "bin"])
def test_load_audio_encoder_reads_a_checkpoint_directory(tmp_path, monkeypatch, fmt):
    """config.json + model.safetensors / pytorch_model.bin -> the constructor arguments and the folded fp32 state dict WanAudioEncoder binds.  Binding itself
    needs a device; here bind() is replaced by a recorder (the GPU suite loads the same directory for real)."""
    from svi_hip import checkpoint, encoders
    sd = {k: torch.from_numpy(v) for k, v in wc.state_dict(wc.SEEDS["tiny"], wc.TINY, fmt == "bin").items()}
    sd["masked_spec_embed"] = torch.zeros(wc.TINY["hidden"])
    (tmp_path / "config.json").write_text(json.dumps(dict(wc.hf_config(wc.TINY), model_type="wav2vec2")))
    if fmt == "safetensors":
        from safetensors.torch import save_file
        save_file(sd, str(tmp_path / "model.safetensors"))
    else:
        torch.save(sd, str(tmp_path / "pytorch_model.bin"))
    seen = {}
    monkeypatch.setattr(encoders.WanAudioEncoder, "bind", lambda self, state: seen.update(state))
    m = checkpoint.load_audio_encoder(str(tmp_path), device="cpu")
    assert {k: getattr(m, k) for k in wc.TINY} == {**wc.TINY, "eps": pytest.approx(wc.TINY["eps"])}
    want = encoders.fold_weight_norm({k: v for k, v in sd.items() if k != "masked_spec_embed"})
    assert set(seen) == set(want)
    for k in want:
        assert seen[k].dtype == torch.float32 and torch.equal(seen[k], want[k]), k
    with pytest.raises(FileNotFoundError):
        os.remove(str(tmp_path / ("model.safetensors" if fmt == "safetensors" else "pytorch_model.bin")))
        checkpoint.load_audio_encoder(str(tmp_path), device="cpu")
    with pytest.raises(ValueError, match="kernels"):
        encoders.WanAudioEncoder.config_from(dict(wc.hf_config(wc.TINY), conv_kernel=[10, 3, 3, 3, 3, 3, 2]))
