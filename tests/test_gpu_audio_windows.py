"""-m gpu: the clip audio windows cut on the device (svi_audio_windows / svi_dit_audio_slot_windows; svi_hip.audio_windows, WanDiT.stage_audio_windows).

The kernel is a clamped gather plus one rounding to bf16, so everything is compared with torch.equal: against the index rule in plain torch
(tests/audio_window_cases.py, held against the reference's gather + regroup in tests/test_audio_windows_host.py), and — for the slots — against
stage_audio on windows built on the host, through forward_talk3."""
import pytest
import torch

import synth
from audio_window_cases import GPU_CASES, GPU_WIDTHS, host_tuples, windows_torch
from gpu_util import dev, errs

pytestmark = pytest.mark.gpu

CFG, SEED = synth.TINY_DIT_TALK, synth.TALK_SEED
_EMB = {}


def _emb(N, R, dtype):
    """The stream's embedding [N, R] ([N, 12, 768] at the real width), made once per size on the host; values that do not survive the rounding
    to bf16 unchanged, so an fp32 source tests it."""
    key = (N, R)
    if key not in _EMB:
        _EMB[key] = torch.from_numpy(synth.randn(7000 + N, N, R))
    e = _EMB[key].to(dtype)
    return e.reshape(N, 12, 768) if R == 9216 else e


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("R", GPU_WIDTHS)
@pytest.mark.parametrize("N,T,start", GPU_CASES)
def test_windows_are_the_index_rule(N, T, start, R, dtype):
    import svi_hip
    emb = _emb(N, R, dtype)
    want_first, want_latter = windows_torch(emb, start, T)
    first, latter = svi_hip.audio_windows(emb.cuda(), start, T)
    assert first.dtype == latter.dtype == torch.bfloat16
    assert first.shape == want_first.shape and latter.shape == want_latter.shape
    assert torch.equal(first.cpu(), want_first) and torch.equal(latter.cpu(), want_latter)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_second_cut_into_the_same_buffers_leaves_no_stale_row(dtype):
    """The real width, the C entry point on caller-owned buffers with a guard row on either side: cut, poison, cut at another start — every row is the
    second start's, and the guards keep their poison."""
    from svi_hip import _lib as L
    N, T, R = 200, 21, 9216
    emb = _emb(N, R, dtype).cuda()
    code = L.SVI_F32 if dtype == torch.float32 else L.SVI_BF16
    POISON = -7.0
    buf_f = torch.full((1 + 5 + 1, R), POISON, dtype=torch.bfloat16, device="cuda")
    buf_l = torch.full((1 + 8 * (T - 1) + 1, R), POISON, dtype=torch.bfloat16, device="cuda")
    for start in (77, 190, 0):
        buf_f.fill_(POISON)
        buf_l.fill_(POISON)
        L.check(L.lib().svi_audio_windows(emb.data_ptr(), code, N, R, start, T, buf_f[1:].data_ptr(), buf_l[1:].data_ptr(), L.current_stream()), "svi_audio_windows")
        want_first, want_latter = windows_torch(emb.cpu(), start, T)
        assert torch.equal(buf_f[1:6].cpu(), want_first.reshape(5, R)), start
        assert torch.equal(buf_l[1:-1].cpu(), want_latter.reshape(-1, R)), start
        for guard in (buf_f[0], buf_f[-1], buf_l[0], buf_l[-1]):
            assert bool((guard == POISON).all()), start
    # T_latent == 1: no later frames, latter_out may be NULL
    buf_f.fill_(POISON)
    L.check(L.lib().svi_audio_windows(emb.data_ptr(), code, N, R, 5, 1, buf_f[1:].data_ptr(), None, L.current_stream()), "svi_audio_windows")
    assert torch.equal(buf_f[1:6].cpu(), windows_torch(emb.cpu(), 5, 1)[0].reshape(5, R)) and bool((buf_f[-1] == POISON).all())


def _model():
    import svi_hip
    sd = {k: torch.from_numpy(v) for k, v in synth.dit_state_dict(SEED, **CFG).items()}
    return svi_hip.WanDiT.from_state_dict(sd, eps=1e-6, num_heads=synth.num_heads_of(CFG), **CFG)


def _clip(grid):
    f, h, w = grid
    x = dev(synth.randn(SEED + 1, 1, 16, f, 2 * h, 2 * w))
    pos = dev(synth.text_context(SEED + 2, 20, CFG["text_dim"], 13))
    neg = dev(synth.text_context(SEED + 12, 20, CFG["text_dim"], 4))
    kw = dict(clip_feature=dev(synth.randn(SEED + 3, 1, 257, 1280)), y=dev(synth.randn(SEED + 4, 1, 20, f, 2 * h, 2 * w)),
              add_condition=dev(0.5 * synth.randn(SEED + 9, 1, f * h * w, CFG["dim"])))
    return x, pos, neg, kw


def test_slots_staged_from_windows_are_slots_staged_from_host_tuples():
    """stage_audio_windows + forward_talk3 == stage_audio(host-built tuples) + forward_talk3, bit for bit: eagerly, for a given null embedding, and as the
    replay of a graph captured BEFORE the slots were re-staged (the clip boundary of a resident talk loop: nothing moves)."""
    m, ref = _model(), _model()
    grid = synth.TALK_GRID
    T = grid[0]
    x, pos, neg, kw = _clip(grid)
    ts = torch.tensor([637.5], device="cuda")
    emb32 = _emb(30, 9216, torch.float32)
    null32 = 0.25 * _emb(7, 9216, torch.float32)

    def want(emb, start, null=None):
        aud, zero = host_tuples(emb, start, T)
        ref.stage_audio(0, aud)
        ref.stage_audio(1, zero if null is None else host_tuples(null, start, T)[0])
        return ref.forward_talk3(x, ts, pos, neg, **kw)

    def same(got, wanted, what):
        for name, g, w in zip(("cond", "uncond", "drop_text"), got, wanted):
            assert torch.equal(g, w), (what, name, errs(g, w))
    for emb in (emb32, emb32.to(torch.bfloat16)):
        for start in (0, 25):
            m.stage_audio_windows(emb.cuda(), start, T)
            assert m.audio_staged(T)
            same(m.forward_talk3(x, ts, pos, neg, **kw), want(emb, start), (emb.dtype, start))
    w0, w25 = want(emb32, 0), want(emb32, 25)
    assert not torch.equal(w0[0], w25[0]) and not torch.equal(w0[2], w25[2])        # the audio reaches the outputs
    m.stage_audio_windows(emb32.cuda(), 3, T, null_emb=null32.cuda())
    got = m.forward_talk3(x, ts, pos, neg, **kw)
    same(got, want(emb32, 3, null32), "null_emb")
    assert not torch.equal(got[1], want(emb32, 3)[1])                              # slot 1 really took the given null audio
    # ---- a graph of the step, captured with start 0 staged; the slots are then cut for start 25 in place and the graph replayed
    m.context_cache(True)
    try:
        outs = [torch.empty_like(x) for _ in range(3)]
        call = lambda: m.forward_talk3(x, ts, pos, neg, out_cond=outs[0], out_uncond=outs[1], out_drop_text=outs[2], **kw)      # noqa: E731
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m.stage_audio_windows(emb32.cuda(), 0, T)
            call()
        side.synchronize()
        same(outs, w0, "eager on the capture stream")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            call()
        torch.cuda.current_stream().wait_stream(side)
        gen = m.generation()
        m.stage_audio_windows(emb32.cuda(), 25, T)
        assert m.generation() == gen                                                # in place: no allocation, no generation move
        for o in outs:
            o.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        same(outs, w25, "replay after the re-stage")
        m.stage_audio_windows(emb32.cuda(), 0, T)
        g.replay()
        torch.cuda.synchronize()
        same(outs, w0, "replay after staging the first start again")
        assert m.generation() == gen
        del g
    finally:
        m.context_cache(False)
    # another frame count re-allocates and moves the generation, as stage_audio does
    gen = m.generation()
    m.stage_audio_windows(emb32.cuda(), 0, T + 1)
    assert m.generation() != gen and m.audio_staged(T + 1)


def test_python_seams_refuse_what_the_kernel_cannot_take():
    import svi_hip
    m = _model()
    emb = _emb(30, 9216, torch.float32).cuda()
    with pytest.raises(ValueError, match="audio width"):
        m.stage_audio_windows(emb.reshape(30, 24, 384)[:, :12].contiguous(), 0, 3)
    with pytest.raises(RuntimeError, match="start = -1"):
        m.stage_audio_windows(emb, -1, 3)
    with pytest.raises(RuntimeError, match="T_latent = 0"):
        m.stage_audio_windows(emb, 0, 0)
    with pytest.raises(RuntimeError, match="R = 12"):
        svi_hip.audio_windows(emb[:, :1, :12].contiguous(), 0, 3)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        svi_hip.audio_windows(emb.reshape(-1)[2:2 + 29 * 9216].reshape(29, 9216), 0, 3)
