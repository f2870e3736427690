"""The audio encoder's per-handle frame limit and the encoder-attention operator without a GPU: every call here refuses before a launch (no device is
touched), so what is pinned is the boundary — svi_w2v_set_max_frames' range, which limit a request is held to and what the message says, the operator's
refusals by argument, the symbol table, and that the Python side's constants are the library's."""
import ctypes as C
import re

import pytest

import wav2vec_cases as wc
from svi_hip import _lib as L
from test_wav2vec_host import _bind_everything, _handle

NEW = ("svi_w2v_set_max_frames", "svi_encoder_attention_f32")


def _cap():
    from svi_hip.encoders import W2V_FRAME_CAP
    return W2V_FRAME_CAP


def test_new_symbols_are_declared_exported_and_typed():
    from test_abi import declared_symbols
    table = {n: (r, a) for n, r, a in L.SYMBOLS}
    lib = L.lib()
    for n in NEW:
        assert n in declared_symbols() and n in table and hasattr(lib, n), n
        assert table[n][0] is C.c_int32
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    assert table["svi_w2v_set_max_frames"][1] == [vp, i32]
    assert table["svi_encoder_attention_f32"][1] == [vp, i32, vp, i32, vp, i32, vp, i32, i32, i32, i32, i32, f32, i32, vp]
    assert sorted(n for n, _, _ in L.SYMBOLS) == declared_symbols()
    assert lib.svi_abi_version() == 13                                           # additive: the version stays


def test_the_cap_is_at_least_16384_and_the_python_constants_are_the_librarys():
    from svi_hip import ops
    from svi_hip.encoders import W2V_DEFAULT_MAX_FRAMES, WanAudioEncoder
    lib = L.lib()
    cap = _cap()
    assert cap >= 16384 and W2V_DEFAULT_MAX_FRAMES == 2048 and WanAudioEncoder.FRAME_CAP == cap == ops.ENCODER_ATTENTION_MAX_KEYS
    _, h = _handle()
    assert lib.svi_w2v_set_max_frames(h, cap) == 0                               # the cap itself is granted ...
    assert lib.svi_w2v_set_max_frames(h, cap + 1) != 0                           # ... and nothing above it
    assert str(cap) in L.last_error() and "max_frames" in L.last_error()
    lib.svi_w2v_destroy(h)
    # the operator's key cap is the same number
    assert lib.svi_encoder_attention_f32(4096, 64, 4096, 64, 4096, 64, 4096, 64, 1, cap + 1, 1, 64, 1.0, 2, None) != 0
    assert "Lk" in L.last_error() and str(cap) in L.last_error()


def test_set_max_frames_refuses_what_is_out_of_range_and_keeps_the_limit():
    lib = L.lib()
    _, h = _handle()
    _bind_everything(h)
    fwd = lambda n, S: lib.svi_w2v_forward(h, 4096, n, S, 8192, L.SVI_F32, None)      # noqa: E731
    for bad in (0, -1, _cap() + 1, 2 ** 31 - 1):
        assert lib.svi_w2v_set_max_frames(h, bad) != 0, bad
        assert f"max_frames {bad}" in L.last_error()
    assert lib.svi_w2v_set_max_frames(None, 4096) != 0 and "null" in L.last_error()
    # a refused setting changed nothing: the handle still refuses as a fresh one does
    assert fwd(16000 * 90, 2049) != 0 and "2048" in L.last_error() and "81 s" in L.last_error()
    lib.svi_w2v_destroy(h)


def test_a_fresh_handle_refuses_2049_with_todays_message_and_names_the_setting():
    lib = L.lib()
    _, h = _handle()
    _bind_everything(h)
    assert lib.svi_w2v_forward(h, 4096, 16000 * 90, 2049, 8192, L.SVI_F32, None) != 0
    msg = L.last_error()
    assert "2048" in msg and "81 s" in msg and "encode the audio in pieces" in msg and "svi_w2v_set_max_frames" in msg
    assert lib.svi_w2v_forward_stage(h, 4096, 16000 * 90, 2049, 0, 8192, 10, None) != 0
    assert "2048" in L.last_error() and "81 s" in L.last_error() and "svi_w2v_set_max_frames" in L.last_error()
    lib.svi_w2v_destroy(h)


def test_a_raised_handle_holds_requests_to_its_own_limit():
    """At 4096: 4097 frames are refused with the limit in the message; 2049 frames pass the length check — on a handle with nothing bound the refusal is
    then the unbound-weights one, the last check before the device."""
    lib = L.lib()
    _, h = _handle()
    assert lib.svi_w2v_set_max_frames(h, 4096) == 0
    fwd = lambda n, S: lib.svi_w2v_forward(h, 4096, n, S, 8192, L.SVI_F32, None)      # noqa: E731
    stage = lambda n, S: lib.svi_w2v_forward_stage(h, 4096, n, S, 0, 8192, 10, None)  # noqa: E731
    for call in (fwd, stage):
        assert call(16000 * 200, 4097) != 0
        assert "4096" in L.last_error() and "4097" in L.last_error() and "never bound" not in L.last_error()
        assert call(16000 * 90, 2049) == 2 and "never bound" in L.last_error()                # SVI_ERR_UNBOUND: the length check was passed
        assert call(16000 * 180, 4096) == 2 and "never bound" in L.last_error()
    # the limit can come down again, below 2048 too
    assert lib.svi_w2v_set_max_frames(h, 100) == 0
    assert fwd(9600, 101) != 0 and "limit of 100 frames" in L.last_error()
    assert fwd(9600, 15) == 2 and "never bound" in L.last_error()
    assert lib.svi_w2v_set_max_frames(h, 2048) == 0
    assert fwd(16000 * 90, 2049) != 0 and "81 s" in L.last_error()
    lib.svi_w2v_destroy(h)


def test_sample_counts_whose_first_layer_passes_a_launch_are_refused():
    """One thread per value of the first layer's [frames_1, conv_dim] output: 2^32 - 256 values at most.  At 32 channels that is past the 2^31 - 1 sample
    limit (never binding); at 512 channels it is 41 943 044 samples, the 65536 frames of the cap by get_embedding's rule."""
    lib = L.lib()
    cfg = dict(wc.TINY, conv_dim=512)
    _, h = _handle(cfg)
    assert lib.svi_w2v_set_max_frames(h, _cap()) == 0                                 # nothing bound: a request that passes every other check ends there
    fwd = lambda n, S: lib.svi_w2v_forward(h, 4096, n, S, 8192, L.SVI_F32, None)      # noqa: E731
    assert fwd(41943045, 100) == 1 and "first convolution layer" in L.last_error()
    assert fwd(41943044, 65536) == 2 and "never bound" in L.last_error()
    assert int(41943044 / 16000 * 25) == 65536 == _cap()
    lib.svi_w2v_destroy(h)


ATT = dict(Q=4096, ldq=128, K=4096, ldk=128, V=4096, ldv=128, O=4096, ldo=128, Lq=4, Lk=4, heads=2, D=64, scale=0.125, kernel=0)


def _att(**kw):
    a = dict(ATT, **kw)
    return L.lib().svi_encoder_attention_f32(a["Q"], a["ldq"], a["K"], a["ldk"], a["V"], a["ldv"], a["O"], a["ldo"], a["Lq"], a["Lk"], a["heads"], a["D"],
                                             a["scale"], a["kernel"], None)


@pytest.mark.parametrize("arg,value,words", [
    ("D", 48, ("D 48",)), ("D", 0, ("D 0",)), ("D", 256, ("D 256",)),
    ("Q", None, ("null",)), ("K", None, ("null",)), ("V", None, ("null",)), ("O", None, ("null",)),
    ("ldq", 127, ("ldq 127", "128")), ("ldk", 127, ("ldk 127", "128")), ("ldv", 64, ("ldv 64", "128")), ("ldo", 0, ("ldo 0", "128")),
    ("Lq", 0, ("Lq 0",)), ("Lk", 0, ("Lk 0",)), ("heads", 0, ("heads 0",)),
    ("Lk", 65537, ("Lk 65537", "65536")), ("Lq", 65537, ("Lq 65537", "65536")),
    ("kernel", 3, ("kernel 3",)), ("kernel", -1, ("kernel -1",)),
])
def test_the_operator_refuses_by_argument_before_any_launch(arg, value, words):
    assert _att(**{arg: value}) != 0
    for w in words:
        assert w in L.last_error(), (w, L.last_error())


def test_the_resident_kernel_refuses_2049_keys_by_name():
    assert _att(kernel=1, Lk=2049) != 0
    assert "kernel 1" in L.last_error() and "2048" in L.last_error() and "2049" in L.last_error()


def test_the_python_operator_checks_its_tensors_on_the_host():
    import torch
    from svi_hip import ops
    q = torch.zeros(4, 2, 64)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.encoder_attention(q, q, q)
    assert ops.ENCODER_ATTENTION_KERNELS == {"auto": 0, "resident": 1, "streaming": 2}
    assert ops.ENCODER_ATTENTION_KEY_TILE >= 64 and ops.ENCODER_ATTENTION_RESIDENT_KEYS == 2048


def test_the_python_constants_are_the_sources():
    """ENC_KT, W2V_FRAME_CAP and W2V_MAX_FRAMES as the sources define them."""
    import os
    from conftest import ROOT
    from svi_hip import ops
    from svi_hip.encoders import W2V_DEFAULT_MAX_FRAMES, W2V_FRAME_CAP
    csrc = os.path.join(ROOT, "stable-video-infinity_amd", "csrc")
    w2v = open(os.path.join(csrc, "svi_wav2vec.hip")).read()
    kernels = open(os.path.join(csrc, "svi_encoder_kernels.hip")).read()
    assert int(re.search(r"#define ENC_KT (\d+)", kernels).group(1)) == ops.ENCODER_ATTENTION_KEY_TILE
    assert int(re.search(r"constexpr int W2V_FRAME_CAP = (\d+);", w2v).group(1)) == W2V_FRAME_CAP
    assert int(re.search(r"constexpr int W2V_MAX_FRAMES = (\d+);", w2v).group(1)) == W2V_DEFAULT_MAX_FRAMES


def test_the_example_names_its_flag_when_the_audio_is_too_long():
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("svi_talk_audio_hip_under_test", os.path.join(ROOT, "examples", "svi_talk_audio_hip.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)

    class Enc:
        FRAME_CAP, max_frames = 65536, 2048
        seq_len = staticmethod(lambda n, sr=16000: int(n / sr * 25))
    ex.check_audio_length(Enc(), 16000 * 81)                                     # 2025 frames: served
    with pytest.raises(SystemExit, match=r"--max_audio_frames 2100"):
        ex.check_audio_length(Enc(), 16000 * 84)
    args = ex.parse_args(["--synthetic", "--max_audio_frames", "4096"])
    assert args.max_audio_frames == 4096 and ex.parse_args(["--synthetic"]).max_audio_frames is None
