"""-m gpu: the streaming fp32 encoder attention (csrc/svi_wav2vec.hip enc_attention_stream_kernel) through its operator seam
(svi_hip.ops.encoder_attention, svi_encoder_attention_f32).

Reference: softmax(scale q k^T) v per head in torch float64 on the CPU, from the same fp32 operands.  gap = max|torch fp32 CPU - float64| of that case, the
bound is wav2vec_cases.bound(gap, rms) = 4 gap + 1e-6 rms: made of the reference's own rounding error, never of what the device computed.  Where the exact
result is known without any rounding (one key that outweighs the rest by e^120: every other term is an exact zero in fp32) the device's row must be that V row
bit for bit.  Every figure is written to the parity report before it is asserted.

KT, the streaming kernel's key tile, is read from svi_hip.ops, so the cases around a tile edge follow the kernel."""
import functools

import numpy as np
import pytest
import torch

import wav2vec_cases as wc
from gpu_util import report

pytestmark = pytest.mark.gpu

HEADS = 2
DS = (32, 64, 80, 128)


def _kt():
    from svi_hip import ops
    return ops.ENCODER_ATTENTION_KEY_TILE


def _reference(q, k, v, scale):
    """q [Lq, H, D], k, v [Lk, H, D] fp32 on the CPU -> (float64 result, gap of torch's fp32 run, rms)."""
    def run(dt):
        s = torch.einsum("qhd,khd->hqk", q.to(dt), k.to(dt)) * scale
        return torch.einsum("hqk,khd->qhd", torch.softmax(s, dim=-1), v.to(dt))
    r64, r32 = run(torch.float64), run(torch.float32)
    return r64, float((r32.double() - r64).abs().max()), float(r64.pow(2).mean().sqrt())


@functools.lru_cache(maxsize=None)
def _gaussian(D, Lq, Lk, seed=0):
    g = torch.Generator().manual_seed(7000 + 131 * D + 17 * Lq + Lk + seed)
    q, k, v = (torch.randn(n, HEADS, D, generator=g) for n in (Lq, Lk, Lk))
    return (q, k, v) + _reference(q, k, v, D ** -0.5)


def _held(tag, got, r64, gap, rms):
    g = got.detach().cpu()
    assert g.dtype == torch.float32 and g.shape == r64.shape
    err = float((g.double() - r64).abs().max()) if bool(torch.isfinite(g).all()) else float("inf")
    b = wc.bound(gap, rms)
    report(f"enc_attention_long_{tag}", max_abs=err, gap=gap, rms=rms, bound=b)
    print(f"enc_attention_long_{tag}: max_abs {err:.3e} gap {gap:.3e} rms {rms:.4f} bound {b:.3e}")
    assert err <= b, (tag, err, gap, b)


def _lk_cases():
    kt = _kt()
    return sorted({1, 2049, 2100, kt - 1, kt, kt + 1, 2 * kt + 1})


@pytest.mark.parametrize("D", DS)
def test_streaming_kernel_against_float64_over_key_counts(D):
    """Lk: one key, the first two sizes the audio encoder sends this way, and every side of a tile edge; 33 query rows = two whole groups and one row."""
    from svi_hip import ops
    for Lk in _lk_cases():
        q, k, v, r64, gap, rms = _gaussian(D, 33, Lk)
        _held(f"D{D}_Lq33_Lk{Lk}", ops.encoder_attention(q.cuda(), k.cuda(), v.cuda(), kernel=2), r64, gap, rms)


@pytest.mark.parametrize("D", DS)
def test_streaming_kernel_against_float64_over_query_counts(D):
    """Lq 1, 15, 17, 33: a lone row, a ragged only group, a group and one row, two groups and one row — at a key count with a ragged last tile."""
    from svi_hip import ops
    Lk = 2 * _kt() + 1
    for Lq in (1, 15, 17, 33):
        q, k, v, r64, gap, rms = _gaussian(D, Lq, Lk)
        _held(f"D{D}_Lq{Lq}_Lk{Lk}", ops.encoder_attention(q.cuda(), k.cuda(), v.cuda(), kernel=2), r64, gap, rms)


@pytest.mark.parametrize("D", DS)
def test_streaming_and_resident_kernels_below_the_threshold(D):
    """Where both kernels run, both are within the bound of float64."""
    from svi_hip import ops
    for Lk in (1, 511, 2048):
        q, k, v, r64, gap, rms = _gaussian(D, 17, Lk)
        for kernel, name in ((1, "resident"), (2, "streaming")):
            _held(f"D{D}_Lk{Lk}_{name}", ops.encoder_attention(q.cuda(), k.cuda(), v.cuda(), kernel=kernel), r64, gap, rms)


def test_kernel_0_is_the_resident_kernel_to_2048_keys_and_the_streaming_one_above():
    from svi_hip import ops
    for Lk, same, name in ((2048, 1, "resident"), (2049, 2, "streaming")):
        q, k, v = (t.cuda() for t in _gaussian(64, 17, Lk)[:3])
        auto = ops.encoder_attention(q, k, v, kernel=0)
        assert torch.equal(auto, ops.encoder_attention(q, k, v, kernel=same)), (Lk, name)
        assert torch.equal(auto, ops.encoder_attention(q, k, v, kernel="auto")) and torch.equal(auto, ops.encoder_attention(q, k, v, kernel=name))
    q, k, v = (t.cuda() for t in _gaussian(64, 17, 2048)[:3])
    assert not torch.equal(ops.encoder_attention(q, k, v, kernel=1), ops.encoder_attention(q, k, v, kernel=2))    # two kernels, two summation orders


def _exact_case(D, Lk, keys):
    """Row i's query is 16 e_0-scaled so that its score is 160 at key keys[i] and 0 at every other key (scale 1): exp(-160) is an exact zero in fp32 whatever
    the running maximum was before.  V row j is filled with j + 1 + channel / 1024 (exact in fp32), so a row says which key it came from."""
    Lq = len(keys)
    q = torch.zeros(Lq, HEADS, D)
    k = torch.zeros(Lk, HEADS, D)
    for i, key in enumerate(keys):
        # one channel per query row, shared by no other row: key `key` has 10 there, the query 16
        q[i, :, i] = 16.0
        k[key, :, i] = 10.0
    v = (torch.arange(Lk, dtype=torch.float32)[:, None, None] + 1.0) + (torch.arange(D, dtype=torch.float32) / 1024.0)[None, None, :] + torch.zeros(1, HEADS, 1)
    v[:, 1] = -v[:, 1]                                                               # the second head's rows differ from the first's
    return q, k, v


@pytest.mark.parametrize("D", DS)
def test_one_dominant_key_gives_its_v_row_bit_for_bit(D):
    """The key that carries the whole row sits where the rescaling can go wrong: the first key; the last key of tile 0; the first key of tile 1 (the maximum
    moves after a whole tile was accumulated: that tile's sum must be scaled to an exact zero); the last key overall and another key of the ragged last tile
    (the maximum arrives only in the last tile); the middle of tile 1 (later tiles underflow completely).  Two rows share key 0's tile to see alpha = 1."""
    from svi_hip import ops
    kt = _kt()
    Lk = 2 * kt + 37
    keys = [0, kt - 1, kt, Lk - 1, 2 * kt + 5, kt + kt // 2, 3, 2 * kt]
    q, k, v = _exact_case(D, Lk, keys)
    r64, gap, rms = _reference(q, k, v, 1.0)
    want = v[keys]
    assert torch.equal(r64.float(), want)                                            # the reference agrees that nothing else contributes
    for kernel in (2, 0):
        got = ops.encoder_attention(q.cuda(), k.cuda(), v.cuda(), scale=1.0, kernel=kernel).cpu()
        wrong = [(i, keys[i]) for i in range(len(keys)) if not torch.equal(got[i], want[i])]
        report(f"enc_attention_long_exact_D{D}_kernel{kernel}", wrong_rows=len(wrong))
        assert not wrong, (kernel, wrong, got[wrong[0][0], 0, :4], want[wrong[0][0], 0, :4])
    # past 2048 keys, where kernel 0 is the streaming kernel: the same placements and the very last key
    Lk = 2048 + 2 * kt + 37
    keys = [0, kt - 1, kt, Lk - 1, Lk - 20, 2048, 8 * kt - 1, 8 * kt]
    q, k, v = _exact_case(D, Lk, keys)
    got = ops.encoder_attention(q.cuda(), k.cuda(), v.cuda(), scale=1.0, kernel=0).cpu()
    assert torch.equal(got, v[keys])


@pytest.mark.parametrize("D", (64, 80))
def test_equal_scores_average_and_a_first_tile_far_below_the_rest(D):
    from svi_hip import ops
    kt = _kt()
    Lk = 2 * kt + 9
    g = torch.Generator().manual_seed(7100 + D)
    # every score equal (q = 0): the uniform average of V
    q, k, v = torch.zeros(17, HEADS, D), torch.randn(Lk, HEADS, D, generator=g), torch.randn(Lk, HEADS, D, generator=g)
    r64, gap, rms = _reference(q, k, v, 1.0)
    assert float((r64 - v.double().mean(dim=0, keepdim=True)).abs().max()) < 1e-12
    _held(f"uniform_D{D}", ops.encoder_attention(q.cuda(), k.cuda(), v.cuda(), scale=1.0, kernel=2), r64, gap, rms)
    # the whole first tile scores -1e30 (finite: the running maximum starts there and then moves by 1e30), the rest are Gaussian scores
    q = torch.randn(17, HEADS, D, generator=g)
    q[:, :, 0] = 1e15
    k = torch.randn(Lk, HEADS, D, generator=g)
    k[:, :, 0] = 0.0
    k[:kt, :, 0] = -1e15
    r64, gap, rms = _reference(q, k, v, 1.0)
    tail, _, _ = _reference(q, k[kt:], v[kt:], 1.0)
    assert float((r64 - tail).abs().max()) < 1e-12                                   # the first tile weighs nothing in the reference
    _held(f"first_tile_far_below_D{D}", ops.encoder_attention(q.cuda(), k.cuda(), v.cuda(), scale=1.0, kernel=2), r64, gap, rms)
    # and -inf itself in the first tile: scores of -inf are the kernel's own padding value, a row's maximum stays -inf for a whole tile
    k[:kt, :, 0] = -float("inf")
    q[:, :, 0] = 1.0
    k[kt:, :, 0] = 0.5
    r64, gap, rms = _reference(q, k, v, 1.0)
    assert bool(torch.isfinite(r64).all())
    _held(f"first_tile_minus_inf_D{D}", ops.encoder_attention(q.cuda(), k.cuda(), v.cuda(), scale=1.0, kernel=2), r64, gap, rms)


@pytest.mark.parametrize("D", DS)
def test_strided_operands_and_nothing_written_outside_the_output(D):
    """q | k | v side by side in one [L, 3 heads D] buffer, as the audio encoder's blocks pass them, and an output inside a wider, longer, poisoned buffer:
    the result is the contiguous call's bit for bit, the poison is untouched."""
    from svi_hip import ops
    L, W = 2 * _kt() + 1, HEADS * D
    q, k, v, r64, gap, rms = _gaussian(D, L, L, seed=5)
    qkv = torch.cat([q.reshape(L, W), k.reshape(L, W), v.reshape(L, W)], dim=1).cuda()
    views = [qkv[:, i * W:(i + 1) * W].unflatten(1, (HEADS, D)) for i in range(3)]
    assert views[1].stride() == (3 * W, D, 1) and views[1].data_ptr() == qkv.data_ptr() + 4 * W
    POISON = -7.25e9
    buf = torch.full((L + 5, W + 24), POISON, device="cuda")
    out = buf[2:2 + L, 8:8 + W].unflatten(1, (HEADS, D))
    got = ops.encoder_attention(*views, kernel=2, out=out)
    assert got.data_ptr() == out.data_ptr()
    inside = buf[2:2 + L, 8:8 + W].clone()
    buf[2:2 + L, 8:8 + W] = POISON
    assert bool((buf == POISON).all()), "the kernel wrote outside [Lq, heads * D]"
    assert torch.equal(inside.unflatten(1, (HEADS, D)), ops.encoder_attention(q.cuda(), k.cuda(), v.cuda(), kernel=2))
    _held(f"strided_D{D}", inside.unflatten(1, (HEADS, D)), r64, gap, rms)
    # a shorter query block against all keys, as a sharded caller would pass it
    part = ops.encoder_attention(views[0][40:57], views[1], views[2], kernel=2)
    assert torch.equal(part, inside.unflatten(1, (HEADS, D))[40:57])


def test_refusals_name_their_argument():
    from svi_hip import ops
    z = lambda n, d=64: torch.zeros(n, HEADS, d, device="cuda")       # noqa: E731
    with pytest.raises(RuntimeError, match="D 48"):
        ops.encoder_attention(z(4, 48), z(4, 48), z(4, 48))
    with pytest.raises(RuntimeError, match="ldk 64"):
        ops.encoder_attention(z(4), torch.as_strided(z(4), (4, HEADS, 64), (64, 64, 1)), z(4))
    with pytest.raises(RuntimeError, match="Lk 65537"):
        ops.encoder_attention(z(4), z(65537), z(65537), kernel=2)
    with pytest.raises(RuntimeError, match="kernel 1.*2048"):
        ops.encoder_attention(z(4), z(2049), z(2049), kernel=1)
    with pytest.raises(TypeError):
        ops.encoder_attention(z(4).bfloat16(), z(4), z(4))
    with pytest.raises(ValueError):
        ops.encoder_attention(z(4), z(5), z(4))
