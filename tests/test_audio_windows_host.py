"""Without a GPU: the clip audio windows' index rule (include/svi_hip.h, svi_audio_windows) is the reference's get_audio_embedding + preprocess_audio,
and the two C entry points refuse bad arguments by name before anything is launched."""
import ctypes as C
import random

import pytest
import torch

from audio_window_cases import GPU_CASES, window_rows, windows_einops, windows_torch
from svi_hip import _lib as L


def _cases():
    """Random N in 1..40, T in 1..4, and for each pair starts on both sides of both clamps: 0 and 1 (the window's left edge is clamped / just is not:
    rows start - 2 .. < 0), around N - 1 - frames (the right edge), around N - 1 (the centre itself passes the end) and far past the end."""
    rnd = random.Random(7)
    out = set(GPU_CASES)
    for _ in range(60):
        N, T = rnd.randint(1, 40), rnd.randint(1, 4)
        frames = 4 * (T - 1) + 1
        for start in (0, 1, 2, 3, N - frames - 3, N - frames - 2, N - frames - 1, N - frames, N - 2, N - 1, N, N + 5, rnd.randint(0, 60)):
            if start >= 0:
                out.add((N, T, start))
    return sorted(out)


def test_index_rule_is_the_reference_gather_and_regroup():
    cases = _cases()
    assert len(cases) > 300
    low = high = 0
    for N, T, start in cases:
        emb = torch.randn(N, 2, 8, generator=torch.Generator().manual_seed(N * 1000 + T * 100 + start))
        first, latter = windows_torch(emb, start, T)
        ref_first, ref_latter = windows_einops(emb, start, T)
        assert tuple(ref_first.shape) == (1, 1, 5, 2, 8) and tuple(ref_latter.shape) == (1, T - 1, 8, 2, 8)
        assert torch.equal(first, ref_first[0]) and torch.equal(latter, ref_latter[0]), (N, T, start)
        low += start < 2
        high += start + 4 * (T - 1) + 2 > N - 1
    assert low > 50 and high > 50              # both clamps were exercised, and so was the unclamped middle
    assert low + high < 2 * len(cases)


def test_rows_of_the_written_out_cases():
    """The rule, spelled out on small cases by hand."""
    first, latter = window_rows(30, 3, 0)
    assert first.tolist() == [0, 0, 0, 1, 2]                                   # video frame 0: rows -2, -1 clamp to 0
    assert latter.tolist() == [[0, 0, 1, 2, 3, 4, 5, 6], [3, 4, 5, 6, 7, 8, 9, 10]]      # frames 1..4: positions 0-2 of 1, centres of 2 and 3, 2-4 of 4
    first, latter = window_rows(30, 3, 25)
    assert first.tolist() == [23, 24, 25, 26, 27]
    assert latter.tolist() == [[24, 25, 26, 27, 28, 29, 29, 29], [28, 29, 29, 29, 29, 29, 29, 29]]      # the high clamp holds the last row
    first, latter = window_rows(1, 2, 0)
    assert first.tolist() == [0] * 5 and latter.tolist() == [[0] * 8]


def _talk_handle():
    cfg = L.DitConfig(256, 36, 512, 16, 64, 256, 1e-6, 1, 2, 2, 2, 2, 1, 1)
    h = C.c_void_p()
    assert L.lib().svi_dit_create(C.byref(cfg), C.byref(h)) == 0
    return h


def test_c_entry_points_refuse_bad_arguments_before_any_launch():
    lib = L.lib()
    P, Q = 4096, 8192                           # never dereferenced: every call below is refused on its arguments
    ok = dict(emb=P, dtype=L.SVI_F32, N=10, R=9216, start=0, T=3, first=Q, latter=Q + 4096)

    def windows(**over):
        a = dict(ok, **over)
        return lib.svi_audio_windows(a["emb"], a["dtype"], a["N"], a["R"], a["start"], a["T"], a["first"], a["latter"], None)
    for over, word in ((dict(emb=None), "emb is NULL"), (dict(N=0), "N = 0"), (dict(T=0), "T_latent = 0"), (dict(R=9217), "R = 9217"), (dict(R=0), "R = 0"),
                       (dict(start=-1), "start = -1"), (dict(dtype=L.SVI_F16), "fp32 or bf16"), (dict(first=None), "NULL output"),
                       (dict(latter=None), "NULL output")):
        assert windows(**over) == 1, over
        assert word in L.last_error(), (over, L.last_error())
    h = _talk_handle()
    try:
        slot = lambda slot=0, emb=P, dtype=L.SVI_BF16, N=10, start=0, T=3: lib.svi_dit_audio_slot_windows(h, slot, emb, dtype, N, start, T, None)      # noqa: E731
        for kw, word in ((dict(emb=None), "emb is NULL"), (dict(N=0), "N = 0"), (dict(T=0), "T_latent = 0"), (dict(start=-3), "start = -3"),
                         (dict(slot=2), "slot 2"), (dict(dtype=L.SVI_F16), "fp32 or bf16"), (dict(emb=P + 4), "16-byte aligned")):
            assert slot(**kw) == 1, kw
            assert word in L.last_error(), (kw, L.last_error())
    finally:
        lib.svi_dit_destroy(h)
    plain = C.c_void_p()
    cfg = L.DitConfig(128, 16, 256, 16, 64, 256, 1e-6, 1, 2, 2, 1, 2, 0, 0)
    assert lib.svi_dit_create(C.byref(cfg), C.byref(plain)) == 0
    assert lib.svi_dit_audio_slot_windows(plain, 0, P, L.SVI_F32, 10, 0, 3, None) == 1 and "enable_multitalk" in L.last_error()
    lib.svi_dit_destroy(plain)


def test_audio_windows_fail_loudly_without_gpu():
    """As test_abi's test_ops_fail_loudly_without_gpu expects of every op: a host tensor is refused by the Python seam, and the C entry point itself,
    given valid arguments on a box without a device, returns an error instead of pretending."""
    import svi_hip
    with pytest.raises(RuntimeError, match="GPU"):
        svi_hip.audio_windows(torch.zeros(4, 12, 768), 0, 2)
    if not torch.cuda.is_available():
        emb, first, latter = torch.zeros(4, 8), torch.zeros(5, 8, dtype=torch.bfloat16), torch.zeros(8, 8, dtype=torch.bfloat16)
        status = L.lib().svi_audio_windows(emb.data_ptr(), L.SVI_F32, 4, 8, 0, 2, first.data_ptr(), latter.data_ptr(), None)
        assert status != 0 and L.last_error()
