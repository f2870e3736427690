"""-m gpu: the bf16 GEMMs that read e4m3 weights (svi_gemm_bf16_w8, csrc/svi_gemm.hip gemm_e8_nt_kernel / gemm_skinny_w8_kernel).

The widening e4m3 -> bf16 is exact, and the kernels widen between the global load and the LDS write / the matrix instruction of the bf16 kernel they
copy: per output element the fp32 sums and their order are the bf16 twin's.  So everything here is torch.equal, no tolerance:
  widening   A = identity: C is the widened weight itself, every finite byte value and every subnormal, once per stage-one kernel id (0 and 128); -0 comes
             out as +0, as it does from the bf16 GEMM on the widened copy (the accumulator starts at +0);
  NaN        a 0x7F / 0xFF byte makes NaN exactly the output column of its row of W;
  twin       svi_gemm_bf16_w8(A, W8) == svi_gemm_bf16_pair(A, widen(W8)) with the bf16 launch held to the id svi_gemm_w8_plan reports (SVI_GEMM_KERNEL),
             every element of C, over M x N x K reaching every loop edge (rows / columns past the tile, K % 64 != 0, the plain and the deep-prefetch
             loop), ldw > K, a base that is 16 but not 32-byte aligned, every epilogue, W2 / n_split on and off a tile boundary, sel_m / sel_n;
             id 0 (the skinny kernel, which no DiT launch takes) through svi_gemm_bf16_skinny with w8 = 0 / 1;
  refusals   an ldw that is no multiple of 16 and a null W: a status, a message, C untouched."""
import ctypes
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

EPI_BIAS, EPI_GELU_TANH, EPI_GATE_RES, EPI_GELU_ERF, EPI_SILU, EPI_RELU = range(6)
MS, NS, KS = (1, 8, 127, 128, 129, 300), (8, 128, 136, 264), (8, 64, 72, 128, 520)
FINITE = [b for b in range(256) if b & 0x7F != 0x7F]          # the 254 byte values that are not NaN


@pytest.fixture(scope="module")
def L():
    import svi_hip
    assert svi_hip._lib.lib().svi_device_count() >= 1
    return svi_hip._lib


def widen(w8):
    return w8.view(torch.float8_e4m3fn).to(torch.bfloat16)


def random_bytes(gen, *shape):
    b = torch.randint(0, 256, shape, dtype=torch.uint8, generator=gen)
    return torch.where(b & 0x7F == 0x7F, b - 1, b)          # NaN codes -> the largest finite value of the same sign


class Operands:
    """One problem on the device.  W8 lives in a byte arena at an offset of 16 bytes (16- but not 32-byte aligned) with rows of ldw > K bytes; the bf16 twin's
    weight is the widened copy with the same leading dimension in elements.  C starts as a pattern so that elements a launch does not own are seen to keep it."""
    def __init__(self, M, N, K, seed, w8_rows=None):
        gen = torch.Generator().manual_seed(seed)
        self.M, self.N, self.K = M, N, K
        self.lda, self.ldw, self.ldc = K + 8, (K + 15) // 16 * 16 + 16, (N + 7) // 8 * 8 + 8
        self.A = torch.zeros(M, self.lda, dtype=torch.bfloat16)
        self.A[:, :K] = torch.randn(M, K, generator=gen).to(torch.bfloat16)
        rows = random_bytes(gen, N, K) if w8_rows is None else w8_rows
        arena = random_bytes(gen, 16 + N * self.ldw + 32)
        arena[16:16 + N * self.ldw].view(N, self.ldw)[:, :K] = rows
        self.arena8 = arena.cuda()
        assert self.arena8.data_ptr() % 32 == 0
        self.W8 = self.arena8[16:16 + N * self.ldw].view(N, self.ldw)
        self.Wb = widen(self.W8).contiguous()
        self.A = self.A.cuda()
        self.bias_n = torch.randn(N, generator=gen).to(torch.bfloat16).cuda()
        self.bias_m = torch.randn(M, generator=gen).to(torch.bfloat16).cuda()
        self.gate = torch.randn(N, generator=gen).cuda()
        self.res = torch.zeros(M, self.ldc, dtype=torch.bfloat16)
        self.res[:, :N] = torch.randn(M, N, generator=gen).to(torch.bfloat16)
        self.res = self.res.cuda()

    def launch(self, L, w8, epi=EPI_BIAS, bias="n", gate=True, n_split=0, sel_m=0, sel_n=0, ldw=None, null_w=False):
        C = torch.full((self.M, self.ldc), -3.0, dtype=torch.bfloat16, device="cuda")
        W = self.W8 if w8 else self.Wb
        b = {"n": self.bias_n, "m": self.bias_m, None: None}[bias]
        W2 = b2 = None
        if n_split:          # the second matrix: rows n_split .. N of the same arena, its own bias
            W2, b2 = W[n_split:], self.bias_n[n_split:]
        fn = L.lib().svi_gemm_bf16_w8 if w8 else L.lib().svi_gemm_bf16_pair
        st = fn(self.A.data_ptr(), self.lda, None if null_w else W.data_ptr(), self.ldw if ldw is None else ldw, C.data_ptr(), self.ldc, self.M, self.N, self.K,
                L.ptr(b), 1 if bias == "m" else 0, epi, self.gate.data_ptr() if (epi == EPI_GATE_RES and gate) else None,
                self.res.data_ptr() if epi == EPI_GATE_RES else None, self.ldc, L.ptr(W2), L.ptr(b2), n_split, sel_m, sel_n, L.current_stream())
        torch.cuda.synchronize()
        return st, C


def twin_equal(L, op, **kw):
    """The e4m3 launch against the bf16 launch on the widened copy held to the kernel svi_gemm_w8_plan names; every element of C (pads included)."""
    k = ctypes.c_int32(0)
    assert L.lib().svi_gemm_w8_plan(kw.get("sel_m") or op.M, kw.get("sel_n") or op.N, op.K, kw.get("epi", EPI_BIAS), 0, 256, ctypes.byref(k)) == 0
    assert k.value == 128
    st8, C8 = op.launch(L, True, **kw)
    assert st8 == 0, L.last_error()
    L.set_switch("SVI_GEMM_KERNEL", k.value)
    try:
        assert L.gemm_plan(op.M, op.N, op.K, kw.get("epi", EPI_BIAS)) == k.value
        stb, Cb = op.launch(L, False, **kw)
    finally:
        L.set_switch("SVI_GEMM_KERNEL", None)
    assert stb == 0, L.last_error()
    assert not torch.isnan(C8[:, :op.N].float()).any()
    assert torch.equal(C8.view(torch.int16), Cb.view(torch.int16)), (op.M, op.N, op.K, kw, (C8.float() - Cb.float()).abs().max().item())
    assert torch.equal(C8[:, op.N:], torch.full_like(C8[:, op.N:], -3.0))          # pad columns keep their bits


def byte_table(N, K):
    """[N, K] bytes in which every finite value appears (row n, column k holds FINITE[(n * 7 + k) % 254])."""
    idx = (torch.arange(N)[:, None] * 7 + torch.arange(K)[None, :]) % len(FINITE)
    return torch.tensor(FINITE, dtype=torch.uint8)[idx]


@pytest.mark.parametrize("kernel", [128, 0])
def test_widening_of_every_finite_byte(L, kernel):
    """A = identity (M = K = 256), no epilogue: C[m][n] is the widened W8[n][m] itself — all 254 finite values, the subnormals with their bits."""
    n = 256 if kernel == 128 else 128          # (the skinny kernel takes M <= 128 rows: two identity halves)
    rows = byte_table(256, 256)
    assert set(rows.flatten().tolist()) == set(FINITE)
    want = widen(rows).T.contiguous()          # [k = m, n]
    for half in range(256 // n):
        op = Operands(n, 256, 256, 1, w8_rows=rows)
        op.A.zero_()
        op.A[:, half * n:(half + 1) * n] = torch.eye(n, dtype=torch.bfloat16, device="cuda")
        C = torch.full((n, op.ldc), -3.0, dtype=torch.bfloat16, device="cuda")
        if kernel == 128:
            st = L.lib().svi_gemm_bf16_w8(op.A.data_ptr(), op.lda, op.W8.data_ptr(), op.ldw, C.data_ptr(), op.ldc, n, 256, 256, None, 0, EPI_BIAS, None, None, 0,
                                          None, None, 0, 0, 0, L.current_stream())
        else:
            st = L.lib().svi_gemm_bf16_skinny(op.A.data_ptr(), op.lda, op.W8.data_ptr(), op.ldw, C.data_ptr(), op.ldc, n, 256, 256, None, EPI_BIAS, None, None, 0, 1,
                                              L.current_stream())
        torch.cuda.synchronize()
        assert st == 0, L.last_error()
        got, exp = C[:, :256].cpu().view(torch.int16), want[half * n:(half + 1) * n].view(torch.int16).clone()
        # byte 0x80 widens to -0, and a GEMM cannot show it: the accumulator starts at +0 and +0 + (-0 * 1) = +0 in IEEE arithmetic, in the bf16 twin on the
        # widened copy as well.  Its output is held to +0 (so -0 is at least not mistaken for a value); every other byte to its exact bits.
        exp[exp == -32768] = 0
        bad = got != exp
        assert not bad.any(), sorted(set(rows.T[half * n:(half + 1) * n][bad].tolist()))          # the byte values that came out wrong


def test_nan_bytes_poison_their_column_only(L):
    M, N, K = 129, 136, 72
    gen = torch.Generator().manual_seed(2)
    rows = random_bytes(gen, N, K)
    rows[5, 3], rows[130, 71] = 0x7F, 0xFF
    op = Operands(M, N, K, 3, w8_rows=rows)
    st, C = op.launch(L, True)
    assert st == 0, L.last_error()
    nan = torch.isnan(C[:, :N].float()).cpu()
    want = torch.zeros(M, N, dtype=torch.bool)
    want[:, 5] = want[:, 130] = True
    assert torch.equal(nan, want)


@pytest.mark.parametrize("M", MS)
def test_twin_every_size(L, M):
    """Every N x K for this M, the epilogue and bias kind walking through all of them."""
    kinds = [dict(epi=EPI_BIAS), dict(epi=EPI_BIAS, bias="m"), dict(epi=EPI_GELU_TANH), dict(epi=EPI_GATE_RES), dict(epi=EPI_BIAS, bias=None),
             dict(epi=EPI_GATE_RES, gate=False)]
    for i, (N, K) in enumerate(itertools.product(NS, KS)):
        twin_equal(L, Operands(M, N, K, 100 + i), **kinds[(i + M) % len(kinds)])


@pytest.mark.parametrize("epi", [EPI_BIAS, EPI_GELU_TANH, EPI_GATE_RES, EPI_GELU_ERF, EPI_SILU, EPI_RELU])
@pytest.mark.parametrize("bias", ["n", "m"])
def test_twin_every_epilogue(L, epi, bias):
    twin_equal(L, Operands(129, 136, 520, 7), epi=epi, bias=bias)
    twin_equal(L, Operands(300, 264, 128, 8), epi=epi, bias=bias)


@pytest.mark.parametrize("K", [256, 576])
def test_twin_both_loops(L, K):
    """K % 64 == 0 and K >= 256 on at most one workgroup per CU: the deep-prefetch loop by default (also with sel_m / sel_n set, as the DiT's stacked
    launches have them); SVI_GEMM_PF = 1 holds both launches to the plain loop."""
    for M, N in ((300, 264), (127, 136)):
        twin_equal(L, Operands(M, N, K, 9), epi=EPI_GATE_RES)
        twin_equal(L, Operands(M, N, K, 10), sel_m=M // 2, sel_n=N)
        L.set_switch("SVI_GEMM_PF", 1)
        try:
            twin_equal(L, Operands(M, N, K, 11), epi=EPI_GELU_TANH)
        finally:
            L.set_switch("SVI_GEMM_PF", None)


@pytest.mark.parametrize("n_split", [128, 136])
def test_twin_weight_pair(L, n_split):
    """W2 / n_split on a tile boundary (one launch, the second matrix through the moved base) and off it (one launch per matrix)."""
    for K in (72, 520, 256):
        twin_equal(L, Operands(129, 264, K, 12), n_split=n_split, sel_n=n_split)
        twin_equal(L, Operands(300, 256 if n_split == 128 else 272, K, 13), n_split=n_split, sel_n=n_split, sel_m=150)


@pytest.mark.parametrize("M", [1, 16, 17, 64, 128])
@pytest.mark.parametrize("K", [128, 256, 1152])
def test_twin_skinny(L, M, K):
    """Plan id 0: both K splits (four and eight waves), the unrolled and the tail loop, every row-block count; bias, and gate + residual."""
    for N, epi in ((136, EPI_BIAS), (264, EPI_GATE_RES)):
        assert L.gemm_plan(M, N, K, epi, skinny=True) == 0
        k = ctypes.c_int32(-1)
        assert L.lib().svi_gemm_w8_plan(M, N, K, epi, 1, 256, ctypes.byref(k)) == 0 and k.value == 0
        op = Operands(M, N, K, 20 + M)
        out = []
        for w8 in (1, 0):
            C = torch.full((M, op.ldc), -3.0, dtype=torch.bfloat16, device="cuda")
            st = L.lib().svi_gemm_bf16_skinny(op.A.data_ptr(), op.lda, (op.W8 if w8 else op.Wb).data_ptr(), op.ldw, C.data_ptr(), op.ldc, M, N, K,
                                              op.bias_n.data_ptr(), epi, op.gate.data_ptr() if epi == EPI_GATE_RES else None,
                                              op.res.data_ptr() if epi == EPI_GATE_RES else None, op.ldc, w8, L.current_stream())
            torch.cuda.synchronize()
            assert st == 0, L.last_error()
            out.append(C)
        assert not torch.isnan(out[0][:, :N].float()).any()
        assert torch.equal(out[0].view(torch.int16), out[1].view(torch.int16))
        assert torch.equal(out[0][:, N:], torch.full_like(out[0][:, N:], -3.0))


def test_refusals(L):
    op = Operands(8, 8, 64, 30)
    st, C = op.launch(L, True, ldw=op.ldw + 8)
    assert st != 0 and "16" in L.last_error()
    assert torch.equal(C, torch.full_like(C, -3.0))
    st, C = op.launch(L, True, null_w=True)
    assert st != 0 and "null" in L.last_error()
    assert torch.equal(C, torch.full_like(C, -3.0))
