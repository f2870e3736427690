"""-m gpu: the audio encoder on the device (svi_hip.WanAudioEncoder, csrc/svi_wav2vec.hip) against the reference's own class run on the CPU
(tests/golden/wav2vec_tiny.npz, wav2vec_base1.npz; tests/gen_golden_wav2vec.py).

Bound, per tensor: max|device - reference fp32| <= 4 x gap + 1e-6 x rms (wav2vec_cases.bound), gap = max|reference fp32 - reference float64| of that tensor
as the fixture recorded it.  It is made of the reference's own rounding error and nothing the device computed; the factor covers a summation order other than
the reference's.  Every figure is written to the parity report before it is asserted.

Measured on an MI355X when this file was written: see profiles/wav2vec_parity.txt."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import synth
import wav2vec_cases as wc
from conftest import ROOT
from gpu_util import dev, host, report

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden")


@functools.lru_cache(maxsize=None)
def _fixture(name):
    return dict(np.load(os.path.join(GOLD, f"wav2vec_{name}.npz")))


@functools.lru_cache(maxsize=None)
def _encoder(name):
    import svi_hip
    cfg = dict(tiny=wc.TINY, base1=wc.BASE1, talk_tiny=wc.TALK_TINY)[name]
    sd = {k: torch.from_numpy(v) for k, v in wc.state_dict(wc.SEEDS[name], cfg).items()}
    return svi_hip.WanAudioEncoder.from_state_dict(sd, wc.hf_config(cfg))


def _check(tag, got, fx, key, rows=None):
    want, gap, rms = fx[key], float(fx[key + ".gap"]), float(fx[key + ".rms"])
    g = host(got).numpy()
    if rows is not None:
        g = g[rows]
    assert g.shape == want.shape and g.dtype == np.float32, (g.shape, want.shape)
    err = float(np.abs(g.astype(np.float64) - want.astype(np.float64)).max()) if np.isfinite(g).all() else float("inf")
    b = wc.bound(gap, rms)
    report(f"wav2vec_{tag}", max_abs=err, gap=gap, rms=rms, bound=b, ratio_to_gap=err / gap)
    print(f"wav2vec_{tag}: max_abs {err:.3e} gap {gap:.3e} rms {rms:.4f} bound {b:.3e}")
    assert err <= b, (tag, err, gap, b)


def _stage_arg(stage):
    if stage.startswith("conv"):
        return ("conv", int(stage[4:]))
    if stage.startswith("layer"):
        return ("layer", int(stage[5:]))
    return stage


STAGES_A = ["wave"] + [f"conv{i}" for i in range(7)] + ["interp", "proj", "pos", "enc_ln", "layer0", "layer1"]
STAGES_REST = ["wave", "conv6", "interp", "proj", "pos", "enc_ln", "layer0", "layer1"]
STAGE_CASES = [("a", s) for s in STAGES_A] + [(i, s) for i in "bcdef" for s in STAGES_REST]


@pytest.mark.parametrize("inp,stage", STAGE_CASES, ids=[f"{i}-{s}" for i, s in STAGE_CASES])
def test_stage_against_the_reference(inp, stage):
    """Every intermediate of the tiny model: a 0.6 s; b 0.25 s; c the same asked for 20 frames (upsampling); d, e odd sample counts (ragged last windows);
    f one frame, seq_len 1.  The positional convolution's padding exceeds the sequence in all of them."""
    fx = _fixture("tiny")
    got = _encoder("tiny").stage(fx[f"{inp}.samples"], _stage_arg(stage), seq_len=int(fx[f"{inp}.seq_len"]))
    _check(f"tiny_{inp}_{stage}", got, fx, f"{inp}.{stage}")


@pytest.mark.parametrize("inp", list("abcdef"))
def test_final_stack_tiny(inp):
    fx = _fixture("tiny")
    S = int(fx[f"{inp}.seq_len"])
    out = _encoder("tiny").encode(fx[f"{inp}.samples"], seq_len=S)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (S, wc.TINY["num_layers"], wc.TINY["hidden"])
    if inp != "c":
        assert S == wc.seq_len(len(fx[f"{inp}.samples"]))
        assert torch.equal(out, _encoder("tiny").encode(torch.from_numpy(fx[f"{inp}.samples"])))        # seq_len by get_embedding's rule; tensor input
    _check(f"tiny_{inp}_stack", out, fx, f"{inp}.stack")
    for l in range(wc.TINY["num_layers"]):                                                              # the writer put block l's rows at [:, l]
        assert torch.equal(out[:, l], _encoder("tiny").stage(fx[f"{inp}.samples"], ("layer", l), seq_len=S))


def test_base_widths_one_block():
    """512 / 768 / 3072 with 12 heads of 64: the tile loops of the convolution at 512 channels (8 x 8 tiles of 64, 32 input-channel chunks), the positional
    convolution's 48-channel groups (a 64-wide tile three quarters full), the encoder attention at D = 64."""
    fx = _fixture("base1")
    m = _encoder("base1")
    out = m.encode(fx["a.samples"])
    assert tuple(out.shape) == (25, 1, 768)
    _check("base1_conv6", m.stage(fx["a.samples"], ("conv", 6)), fx, "a.conv6", rows=wc.BASE1_ROWS)
    _check("base1_stack", out, fx, "a.stack")


def test_output_dtype_switch():
    fx = _fixture("tiny")
    m = _encoder("tiny")
    f32 = m.encode(fx["a.samples"])
    b16 = m.encode(fx["a.samples"], dtype=torch.bfloat16)
    assert b16.dtype == torch.bfloat16 and b16.shape == f32.shape
    assert torch.equal(b16, f32.to(torch.bfloat16))
    with pytest.raises(ValueError):
        m.encode(fx["a.samples"], dtype=torch.float16)


def test_one_handle_different_lengths_nothing_stale():
    """Long, short, long, then longer than everything before (the workspace grows) and short again: every result is the result of a fresh handle."""
    import svi_hip
    fx = _fixture("tiny")
    sd = {k: torch.from_numpy(v) for k, v in wc.state_dict(wc.SEEDS["tiny"], wc.TINY).items()}
    fresh = lambda: svi_hip.WanAudioEncoder.from_state_dict(sd, wc.hf_config(wc.TINY))      # noqa: E731
    long_x = wc.waveform(21, 20000)
    want = {k: fresh().encode(x).clone() for k, x in (("a", fx["a.samples"]), ("b", fx["b.samples"]), ("f", fx["f.samples"]), ("long", long_x))}
    m = fresh()
    for k, x in (("a", fx["a.samples"]), ("b", fx["b.samples"]), ("a", fx["a.samples"]), ("f", fx["f.samples"]), ("long", long_x), ("b", fx["b.samples"])):
        assert torch.equal(m.encode(x), want[k]), k
    _check("tiny_b_after_others", m.encode(fx["b.samples"]), fx, "b.stack")


def test_refusals_on_the_device_leave_the_output_alone():
    m = _encoder("tiny")
    with pytest.raises(RuntimeError, match="2048"):
        m.encode(np.zeros(16000 * 82 + 100, np.float32))
    with pytest.raises(RuntimeError, match="seq_len 0"):
        m.encode(np.zeros(500, np.float32))
    with pytest.raises(RuntimeError, match="samples"):
        m.encode(np.zeros(0, np.float32))
    with pytest.raises(ValueError):
        m.encode(np.zeros((2, 800), np.float32))
    with pytest.raises(ValueError, match="16 kHz"):
        m.encode(np.zeros(800, np.float32), sr=8000)


@pytest.mark.parametrize("fmt", ["safetensors", "bin"])
def test_checkpoint_directory_and_module_loaders(tmp_path, fmt):
    """load_audio_encoder on a directory written here, and from_module on an object with the Hugging Face model's two members: the same bits as
    from_state_dict, under both spellings of the weight-norm keys."""
    import svi_hip
    fx = _fixture("tiny")
    sd = {k: torch.from_numpy(v) for k, v in wc.state_dict(wc.SEEDS["tiny"], wc.TINY, fmt == "bin").items()}
    (tmp_path / "config.json").write_text(json.dumps(wc.hf_config(wc.TINY)))
    if fmt == "safetensors":
        from safetensors.torch import save_file
        save_file(sd, str(tmp_path / "model.safetensors"))
    else:
        torch.save(sd, str(tmp_path / "pytorch_model.bin"))
    want = _encoder("tiny").encode(fx["a.samples"])
    assert torch.equal(svi_hip.checkpoint.load_audio_encoder(str(tmp_path)).encode(fx["a.samples"]), want)

    class Module:
        config = type("Config", (), wc.hf_config(wc.TINY))()

        def state_dict(self):
            return sd
    assert torch.equal(svi_hip.WanAudioEncoder.from_module(Module()).encode(fx["a.samples"]), want)


def test_talk_stream_encodes_speech_itself():
    """TalkStreamLoop.run(speech=, audio_encoder=) is run(audio_embedding=encoder.encode(speech)), bit for bit, on the tiny talk model of
    tests/test_gpu_talk_stream.py's size: 0.8 s of audio = 20 rows, three clips of 9 frames (the audio ends inside the last)."""
    import svi_hip
    CFG, H, W, NF, STEPS, CLIPS = synth.TINY_DIT_TALK, 32, 48, 9, 2, 3
    sd = {k: torch.from_numpy(v) for k, v in synth.dit_state_dict(synth.TALK_SEED, **CFG).items()}
    dit = svi_hip.WanDiT.from_state_dict(sd, eps=1e-6, num_heads=synth.num_heads_of(CFG), **CFG)
    vae = svi_hip.WanVideoVAE.from_state_dict({k: torch.from_numpy(v) for k, v in synth.vae_state_dict(500).items()})
    img, ref_frame = torch.from_numpy(synth.condition_frames(31, 1, H, W)), torch.from_numpy(synth.condition_frames(32, 1, H, W)[0])
    prompt = (dev(synth.text_context(40, 16, CFG["text_dim"], 9)), dev(synth.text_context(50, 16, CFG["text_dim"], 5)))
    clipf = dev(synth.randn(33, 1, 257, 1280))
    enc = _encoder("talk_tiny")
    speech = wc.waveform(31, 12800)
    emb = enc.encode(speech)
    assert tuple(emb.shape) == (20, 12, 768) and emb.is_cuda and bool(torch.isfinite(emb).all()) and float(emb.std()) > 0.1

    def run(**audio):
        sl = svi_hip.TalkStreamLoop(dit, vae, clip_encoder=lambda first: clipf, num_motion_frames=1, num_frames=NF, num_inference_steps=STEPS,
                                    cfg_scale=dict(audio=4.0, text=5.0), ref_pad_num=-1)
        return sl.run(img, ref_frame, prompt, num_clips=CLIPS, seed=5, **audio), sl.trace
    v_speech, tr_speech = run(speech=speech, audio_encoder=enc)
    v_emb, tr_emb = run(audio_embedding=emb)
    assert v_speech.dtype == torch.uint8 and tuple(v_speech.shape) == (CLIPS * NF, H, W, 3)
    assert torch.equal(v_speech, v_emb)
    for a, b in zip(tr_speech, tr_emb):
        assert torch.equal(a["latents"], b["latents"]) and a["audio_start"] == b["audio_start"]
    v_pos, _ = run(audio_emb=emb.cpu())                                    # the existing spelling, a host tensor: unchanged
    assert torch.equal(v_pos, v_emb)
    with pytest.raises(TypeError):
        run(speech=speech)
    with pytest.raises(TypeError):
        run(speech=speech, audio_encoder=enc, audio_embedding=emb)
    with pytest.raises(TypeError):
        run()


def test_example_launcher_runs_a_synthetic_talk_stream_from_samples(tmp_path):
    """examples/svi_talk_audio_hip.py --synthetic: the talk example's surface with the audio encoder on the device — 3 clips of 9 frames from a synthetic
    waveform, every clip whole, the cursor 0 / 8 / 17, one captured step graph; no Hugging Face model class is imported by the script."""
    import subprocess
    import sys
    script = os.path.join(ROOT, "examples", "svi_talk_audio_hip.py")
    assert "import transformers" not in open(script).read() and "Wav2Vec2" not in open(script).read()
    r = subprocess.run([sys.executable, script, "--synthetic", "--num_clips", "3", "--num_steps", "3", "--height", "32", "--width", "48", "--max_frames", "9",
                        "--output", str(tmp_path), "--ref_pad_num", "-1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    rec = json.loads([l for l in r.stdout.splitlines() if l.startswith('{"svi_talk_audio_hip"')][-1])["svi_talk_audio_hip"][0]
    assert rec["audio_encoder_on_device"] and rec["audio_frames"] == 23                 # 23 * 640 samples; the stream outlasts its audio
    assert rec["clips"] == 3 and rec["frames"] == 27 and rec["audio_starts"] == [0, 8, 17] and rec["step_graph_captures"] == 1
    vid = np.load(os.path.join(rec["out"], "video_u8.npy"))
    assert vid.shape == (27, 32, 48, 3) and vid.dtype == np.uint8 and vid.std() > 0
