"""-m gpu: the 256-row bf16 GEMM that reads e4m3 weights (gemm_w8_nt_256e_kernel, csrc/svi_gemm.hip; plan id 260 of svi_gemm_w8_plan under SVI_GEMM_W8_256 = 1).

It is the twin of gemm_bf16_nt_256e_kernel<2, 256>: same tile, MFMA, k order per element and epilogue, W widened exactly between the LDS read and the matrix
instruction.  So everything here is torch.equal on the int16 view, no tolerance, against svi_gemm_bf16_pair on the widened copy held to id 260.  The 256-row
route is forced at small sizes with SVI_GEMM_KERNEL = 260 beside the switch, and every comparison first asserts through both planners that both launches take
260 — a comparison that ran the 128^2 tile on both sides would prove nothing.
  sizes     K = 64 (one tile: prologue only), 128 (two: no third A stage), 192 (first tile with every stage), 576 (odd count in steady state, buffer flip);
            M = 1, 255, 256, 257, 300 (row edge, second row tile); N = 8, 136, 256, 264, 520 (column edge, second and third column tile, rows past N);
            every N x K for each M, all six epilogues and bias along n / along m / none walking through them; C's pads keep their pattern;
  pair      W2 / n_split on the tile boundary (256: one launch, moved base) and off it (264: two launches), sel_n / sel_m as the DiT's stacked launches set them;
  bytes     A = identity: C is the widened byte itself for every finite code;  a NaN byte poisons exactly its own column;
  off       without SVI_GEMM_W8_256 the same launch plans to 128 and gives the same bits."""
import contextlib
import ctypes
import itertools

import pytest
import torch

from test_gpu_gemm_w8 import FINITE, Operands, byte_table, random_bytes, widen

pytestmark = pytest.mark.gpu

EPI_BIAS, EPI_GELU_TANH, EPI_GATE_RES, EPI_GELU_ERF, EPI_SILU, EPI_RELU = range(6)
MS, NS, KS = (1, 255, 256, 257, 300), (8, 136, 256, 264, 520), (64, 128, 192, 576)
# all six epilogues, bias along n / along m / none, the gate present and absent
KINDS = [dict(epi=EPI_BIAS), dict(epi=EPI_BIAS, bias="m"), dict(epi=EPI_GELU_TANH), dict(epi=EPI_GATE_RES), dict(epi=EPI_BIAS, bias=None),
         dict(epi=EPI_GATE_RES, gate=False), dict(epi=EPI_GELU_ERF, bias="m"), dict(epi=EPI_SILU), dict(epi=EPI_RELU, bias="m"), dict(epi=EPI_GELU_ERF),
         dict(epi=EPI_SILU, bias="m"), dict(epi=EPI_RELU), dict(epi=EPI_GELU_TANH, bias="m")]


@pytest.fixture(scope="module")
def L():
    import svi_hip
    assert svi_hip._lib.lib().svi_device_count() >= 1
    return svi_hip._lib


@contextlib.contextmanager
def switches(L, **kv):
    try:
        for k, v in kv.items():
            L.set_switch(k, v)
        yield
    finally:
        for k in kv:
            L.set_switch(k, None)


def w8_plan(L, M, N, K, epi=EPI_BIAS):
    k = ctypes.c_int32(-1)
    assert L.lib().svi_gemm_w8_plan(M, N, K, epi, 0, 256, ctypes.byref(k)) == 0, L.last_error()
    return k.value


def launch_w8_256(L, op, **kw):
    """The e4m3 launch on the new kernel: SVI_GEMM_KERNEL = 260 and the switch, id 260 asserted on the planner."""
    with switches(L, SVI_GEMM_KERNEL=260, SVI_GEMM_W8_256=1):
        assert w8_plan(L, kw.get("sel_m") or op.M, kw.get("sel_n") or op.N, op.K, kw.get("epi", EPI_BIAS)) == 260
        st, C = op.launch(L, True, **kw)
    assert st == 0, L.last_error()
    return C


def launch_bf16_260(L, op, **kw):
    with switches(L, SVI_GEMM_KERNEL=260):
        assert L.gemm_plan(kw.get("sel_m") or op.M, kw.get("sel_n") or op.N, op.K, kw.get("epi", EPI_BIAS)) == 260
        st, C = op.launch(L, False, **kw)
    assert st == 0, L.last_error()
    return C


def twin_equal(L, op, **kw):
    C8, Cb = launch_w8_256(L, op, **kw), launch_bf16_260(L, op, **kw)
    assert not torch.isnan(C8[:, :op.N].float()).any()
    assert torch.equal(C8.view(torch.int16), Cb.view(torch.int16)), (op.M, op.N, op.K, kw, (C8.float() - Cb.float()).abs().max().item())
    assert torch.equal(C8[:, op.N:], torch.full_like(C8[:, op.N:], -3.0))          # pad columns keep their bits
    return C8


@pytest.mark.parametrize("M", MS)
def test_twin_every_size(L, M):
    """Every N x K for this M, the epilogue and bias kind walking through all of them."""
    for i, (N, K) in enumerate(itertools.product(NS, KS)):
        twin_equal(L, Operands(M, N, K, 300 + i), **KINDS[(i + M) % len(KINDS)])


@pytest.mark.parametrize("epi", [EPI_BIAS, EPI_GELU_TANH, EPI_GATE_RES, EPI_GELU_ERF, EPI_SILU, EPI_RELU])
@pytest.mark.parametrize("bias", ["n", "m", None])
def test_twin_every_epilogue(L, epi, bias):
    twin_equal(L, Operands(257, 264, 192, 17), epi=epi, bias=bias)


@pytest.mark.parametrize("n_split", [256, 264])
@pytest.mark.parametrize("K", [64, 576])
def test_twin_weight_pair(L, n_split, K):
    """W2 / n_split on the 256-wide tile boundary (one launch, the second matrix through the moved base of n_split x ldw BYTES) and off it (one launch per
    matrix); sel_n = n_split and sel_m = the per-sample rows, as the DiT's stacked q | k launch sets them; the last case's
    second matrix has another height (136 rows: rows past N in its last tile)."""
    N = 2 * n_split
    twin_equal(L, Operands(300, N, K, 12), n_split=n_split, sel_n=n_split)
    twin_equal(L, Operands(300, N, K, 13), n_split=n_split, sel_n=n_split, sel_m=150)
    twin_equal(L, Operands(257, n_split + 136, K, 14), n_split=n_split, sel_n=n_split)


def test_widening_of_every_finite_byte(L):
    """A = identity (M = K = 256), N = 256, no bias: C[m][n] is the widened W8[n][m] itself — all 254 finite codes, the subnormals with their bits."""
    rows = byte_table(256, 256)
    assert set(rows.flatten().tolist()) == set(FINITE)
    op = Operands(256, 256, 256, 1, w8_rows=rows)
    op.A.zero_()
    op.A[:, :256] = torch.eye(256, dtype=torch.bfloat16, device="cuda")
    C = launch_w8_256(L, op, bias=None)
    got, exp = C[:, :256].cpu().view(torch.int16), widen(rows).T.contiguous().view(torch.int16).clone()
    exp[exp == -32768] = 0          # byte 0x80 = -0: the accumulator starts at +0 and +0 + (-0 * 1) = +0, in the bf16 twin as well (tests/test_gpu_gemm_w8.py)
    bad = got != exp
    assert not bad.any(), sorted(set(rows.T[bad].tolist()))          # the byte values that came out wrong


def test_nan_bytes_poison_their_column_only(L):
    """One NaN byte in a row of the second column tile, one in the last k of the odd K tile (tile 1 of three: k = 127), one in the last k of all."""
    M, N, K = 257, 520, 192
    rows = random_bytes(torch.Generator().manual_seed(2), N, K)
    rows[300, 70], rows[5, 127], rows[140, 191] = 0x7F, 0xFF, 0x7F
    C = launch_w8_256(L, Operands(M, N, K, 3, w8_rows=rows))
    nan = torch.isnan(C[:, :N].float()).cpu()
    want = torch.zeros(M, N, dtype=torch.bool)
    want[:, 300] = want[:, 5] = want[:, 140] = True
    assert torch.equal(nan, want)


def test_switch_off_keeps_the_128_tile_and_its_bits(L):
    """SVI_GEMM_KERNEL = 260 alone: svi_gemm_bf16_w8 still plans to the 128^2 tile (resident mode's default route is untouched), and its bits are the new
    kernel's."""
    for M, N, K, kw in ((300, 520, 576, dict(epi=EPI_GATE_RES)), (257, 264, 128, dict(epi=EPI_GELU_TANH, bias="m"))):
        op = Operands(M, N, K, 40)
        with switches(L, SVI_GEMM_KERNEL=260):
            assert w8_plan(L, M, N, K, kw["epi"]) == 128 and L.gemm_plan(M, N, K, kw["epi"]) == 260
            st, C128 = op.launch(L, True, **kw)
        assert st == 0, L.last_error()
        assert torch.equal(C128.view(torch.int16), launch_w8_256(L, op, **kw).view(torch.int16))
