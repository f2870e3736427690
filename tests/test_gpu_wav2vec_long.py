"""-m gpu: the audio encoder past 2048 frames (svi_hip.WanAudioEncoder(max_frames=), csrc/svi_wav2vec.hip with its streaming
attention kernel) against the reference's own class run on the CPU (tests/golden/wav2vec_long.npz; tests/gen_golden_wav2vec_long.py).

Bound, per tensor, on the rows the fixture keeps: max|device - reference fp32| <= 4 x gap + 1e-6 x rms (wav2vec_cases.bound), gap = max|reference fp32 -
reference float64| as the fixture recorded it — the bound of tests/test_gpu_wav2vec.py, made of the reference's own rounding error.  Every figure is written
to the parity report before it is asserted.

Measured on an MI355X when this file was written: see profiles/wav2vec_long_parity.txt."""
import functools
import os

import numpy as np
import pytest
import torch

import wav2vec_cases as wc
import wav2vec_long_cases as lc
from conftest import ROOT
from gpu_util import host, report

pytestmark = pytest.mark.gpu

CASES = {name: (which, n, seed, S) for name, which, n, seed, S in lc.LONG_INPUTS}


@functools.lru_cache(maxsize=None)
def _fixture():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "wav2vec_long.npz")))


@functools.lru_cache(maxsize=None)
def _encoder(which, max_frames=lc.MAX_FRAMES):
    import svi_hip
    cfg = dict(tiny=wc.TINY, base1=wc.BASE1)[which]
    sd = {k: torch.from_numpy(v) for k, v in wc.state_dict(wc.SEEDS[which], cfg).items()}
    return svi_hip.WanAudioEncoder.from_state_dict(sd, wc.hf_config(cfg), max_frames=max_frames)


@functools.lru_cache(maxsize=None)
def _speech(name):
    which, n, seed, S = CASES[name]
    fx = _fixture()
    assert int(fx[f"{name}.n_samples"]) == n and int(fx[f"{name}.wave_seed"]) == seed
    assert int(fx[f"{name}.seq_len"]) == (wc.seq_len(n) if S is None else S) > 2048
    return torch.from_numpy(wc.waveform(seed, n)).cuda()


@functools.lru_cache(maxsize=None)
def _stack(name):
    """encode() of a case on the raised handle, computed once and left unchanged."""
    return _encoder(CASES[name][0]).encode(_speech(name), seq_len=int(_fixture()[f"{name}.seq_len"]))


def _check(tag, got, key):
    fx = _fixture()
    want, gap, rms = fx[key], float(fx[key + ".gap"]), float(fx[key + ".rms"])
    g = host(got)
    g = g[torch.from_numpy(lc.kept_rows(g.shape[0]))].numpy()
    assert g.shape == want.shape and g.dtype == np.float32, (g.shape, want.shape)
    err = float(np.abs(g.astype(np.float64) - want.astype(np.float64)).max()) if np.isfinite(g).all() else float("inf")
    b = wc.bound(gap, rms)
    report(f"wav2vec_long_{tag}", max_abs=err, gap=gap, rms=rms, bound=b, ratio_to_gap=err / gap)
    print(f"wav2vec_long_{tag}: max_abs {err:.3e} gap {gap:.3e} rms {rms:.4f} bound {b:.3e}")
    assert err <= b, (tag, err, gap, b)


def _stage_arg(stage):
    return ("conv", int(stage[4:])) if stage.startswith("conv") else stage


STAGE_CASES = [(name, s) for name in "pqr" for s in lc.STAGES[name] if s != "stack"]


@pytest.mark.parametrize("name,stage", STAGE_CASES, ids=[f"{n}-{s}" for n, s in STAGE_CASES])
def test_stage_against_the_reference(name, stage):
    """p: 12 frames interpolated up to 2049; q: 84 s of audio, 268 799 rows after the first layer, statistics over hundreds of chunks; r: base widths."""
    S = int(_fixture()[f"{name}.seq_len"])
    got = _encoder(CASES[name][0]).stage(_speech(name), _stage_arg(stage), seq_len=S)
    _check(f"{name}_{stage}", got, f"{name}.{stage}")


@pytest.mark.parametrize("name", list("pqr"))
def test_final_stack_against_the_reference(name):
    which = CASES[name][0]
    cfg = dict(tiny=wc.TINY, base1=wc.BASE1)[which]
    S = int(_fixture()[f"{name}.seq_len"])
    out = _stack(name)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (S, cfg["num_layers"], cfg["hidden"])
    _check(f"{name}_stack", out, f"{name}.stack")
    for l in range(cfg["num_layers"]):                                                # block l's own output is column l, bit for bit
        assert torch.equal(out[:, l], _encoder(which).stage(_speech(name), ("layer", l), seq_len=S))
    if name == "q":                                                                    # seq_len by get_embedding's rule
        assert torch.equal(out, _encoder(which).encode(_speech(name)))


def test_raising_the_limit_changes_no_bits_at_or_below_2048_frames():
    """The same weights on a default handle and on one raised to 4096: every length a default handle serves comes out bit for bit the same, 2048 included
    (the last size of the resident attention kernel)."""
    raised, default = _encoder("tiny"), _encoder("tiny", None)
    assert raised.max_frames == 4096 and default.max_frames == 2048
    x = torch.from_numpy(wc.waveform(23, 9600)).cuda()
    for S in (15, 700, 2048):
        assert torch.equal(raised.encode(x, seq_len=S), default.encode(x, seq_len=S)), S
    assert torch.equal(raised.stage(x, "enc_ln", seq_len=2048), default.stage(x, "enc_ln", seq_len=2048))
    # and the limit is the handle's: moving it up and down on one handle leaves its results where they were
    want = default.encode(x, seq_len=700).clone()
    default.max_frames = 3000
    assert default.max_frames == 3000 and tuple(default.encode(x, seq_len=2500).shape) == (2500, 2, 128)
    default.max_frames = 2048
    assert torch.equal(default.encode(x, seq_len=700), want)
    with pytest.raises(RuntimeError, match="max_frames"):
        default.max_frames = 0
    assert default.max_frames == 2048


def test_refusals_follow_the_handles_limit():
    x = _speech("q")
    with pytest.raises(RuntimeError, match="2048"):
        _encoder("tiny", None).encode(x)
    with pytest.raises(RuntimeError, match="2099"):
        _encoder("tiny", 2099).encode(x)
    with pytest.raises(RuntimeError, match="2099"):
        _encoder("tiny", 2099).stage(x, "interp")
    assert tuple(_encoder("tiny", 2100).encode(x).shape) == (2100, 2, 128)


def test_a_clip_that_begins_past_frame_2048_gets_its_own_audio():
    """ops.audio_windows on q's 2100 rows at start 2060 (rows 2058 .. 2070, all past 2048) and at 2092 (the clamp holds row 2099): the rows the clamp rule
    names (audio_window_cases.window_rows: the row of video frame f, window position w is emb[clamp(start + f + w - 2, 0, N - 1)]), rounded to bf16."""
    from audio_window_cases import window_rows
    from svi_hip import ops
    emb = _stack("q")
    N, tlat = emb.shape[0], 3
    assert N == 2100
    for start in (2060, 2092):
        first, latter = ops.audio_windows(emb, start, tlat)
        assert tuple(first.shape) == (1, 5, 2, 128) and tuple(latter.shape) == (tlat - 1, 8, 2, 128)
        rf, rl = window_rows(N, tlat, start)
        assert int(rf.min()) == start - 2 > 2048 and int(rl.max()) == min(start + 4 * (tlat - 1) + 2, N - 1)
        assert torch.equal(first, emb[rf.cuda()][None].to(torch.bfloat16)) and torch.equal(latter, emb[rl.cuda()].to(torch.bfloat16))
    assert not torch.equal(emb[2058], emb[2059])                                           # neighbouring rows differ: a wrong row would show


def test_output_dtype_switch_at_2100_frames():
    f32 = _stack("q")
    b16 = _encoder("tiny").encode(_speech("q"), dtype=torch.bfloat16)
    assert b16.dtype == torch.bfloat16 and b16.shape == f32.shape
    assert torch.equal(b16, f32.to(torch.bfloat16))


def test_loaders_pass_the_limit_on(tmp_path):
    import json
    import svi_hip
    from safetensors.torch import save_file
    sd = {k: torch.from_numpy(v) for k, v in wc.state_dict(wc.SEEDS["tiny"], wc.TINY).items()}
    (tmp_path / "config.json").write_text(json.dumps(wc.hf_config(wc.TINY)))
    save_file(sd, str(tmp_path / "model.safetensors"))
    m = svi_hip.checkpoint.load_audio_encoder(str(tmp_path), max_frames=4096)
    assert m.max_frames == 4096 and svi_hip.checkpoint.load_audio_encoder(str(tmp_path)).max_frames == 2048
    assert torch.equal(m.encode(_speech("p"), seq_len=2049), _stack("p"))

    class Module:
        config = type("Config", (), wc.hf_config(wc.TINY))()

        def state_dict(self):
            return sd
    assert svi_hip.WanAudioEncoder.from_module(Module(), max_frames=2100).max_frames == 2100
    assert svi_hip.WanAudioEncoder(**wc.TINY, max_frames=2500).max_frames == 2500 and svi_hip.WanAudioEncoder(**wc.TINY).max_frames == 2048
