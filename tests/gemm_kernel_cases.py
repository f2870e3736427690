"""Case table, inputs, references, emulation, bound and write mask of tests/test_gpu_gemm_kernels.py (no GPU imports): the bf16 GEMM family of
csrc/svi_gemm.hip in the strided forms the DiT launches — through svi_gemm_bf16, svi_linear_row_stats and svi_gemm_bf16_pair (the q | k launch with
W2 / bias2 / n_split, and the stacked pair's sel_m / sel_n).  tests/test_gemm_kernel_cases.py runs all of it on the host.

reference   fp64, rounded to bf16 (rbf = row_kernel_cases.rbf64, ONE rounding) only where the kernels round:
              y1  = rbf(acc + bias)                         bias along N, or along M (bias_along_m); absent = 0
              out = rbf(f(y1))                              f = identity | gelu_tanh | gelu_erf | silu | relu
              out = rbf(res + rbf(gate y1)), rbf(res + y1)  with and without a gate
              row statistic = fp64 sum of squares of the rounded out over each aligned 64-column group
            This is what both epilogues do (svi_gemm.hip, "epilogue part 1 / part 2" of gemm_bf16_nt_kernel, and gemm256_epilogue_t).  Differences found
            between the two, none of which changes a value: the 128^2 kernel adds `acc + bias`, the 256-row one `acc + (bias_n + bias_m)` with one of the
            two terms always 0; the 256-row one fetches bias (8 B) and gate (16 B) as vectors when the tile is whole and the pointer aligned (case
            `n264_misaligned` takes the other branch), loads an interior tile's residual before the read-back, and leaves the row statistic only under
            the plain bias epilogue (the 128^2 kernel under whichever epilogue runs; the launcher admits the plain one only).
emulation   the same in fp32: K in 64-wide tiles, a tile as two k-steps of 32, a k-step as the MFMA's four lane groups of 8 k each (summed one after the
            other), the four group sums added pairwise and then to the accumulator; activations in fp32 by the kernels' formulas.  Not held to be
            bit-exact with the device: it stands for correct fp32 arithmetic in another order.
bound       per element |got - want| <= 2^-8 |want| + C_NOISE 2^-24 S.  S0 = sum_k |a_k w_k| + |bias| is what the accumulation's noise is relative to;
            S = max(S0, |y1|) under an activation (never below |y1|), S = |res| + |gate| max(S0, |y1|) for the residual form (never below
            |res| + |gate y1|; it can cancel: case rows `cancel`).  An element outside the bound but within two bf16 ulps at max(|want|, S) is a MOVED
            ROUNDING, anything further off a failure; moved roundings may be at most MOVED_CAP = 2e-3 of the elements of ANY row.

Inputs.  The cap is per row and the N edges are narrow: in a row of 200 elements ONE moved rounding is 5e-3.  With bf16 Gaussian operands the fp32
accumulation alone moves a rounding in about 2 S0 2^-24 / (|y| 2^-8) = 3e-4 (K = 128) to 1e-3 (K = 1536) of the elements (S0 / |y| = 0.64 sqrt(K)), i.e.
in most rows of every case: no K or spread of such operands stays under the cap.  So the operands are Gaussian values ON A FIXED-POINT GRID — multiples
of 2^-3, at most 4 in magnitude (edge rows: times 2^40, 2^-40, 0) — for which every product and every partial sum up to K = 1536 is an integer multiple
of 2^-6 below 2^21 times one power of two: exact in fp32 IN ANY ORDER.  y1 is then the reference's to the bit, relu / identity / gate (bf16-valued) /
residual add nothing, and only equality meets the bound; what noise is left is the bias added to a 2^-40 row, an fp32 gate (`wide_gate_f32`), and the
fp32 gelu / silu / erf.  One combination is left out because correct fp32 arithmetic itself breaks the cap on it: a 2^40 row's sums are short integers,
one in 16 of them a bf16 tie, and fp32 drops the bias that breaks the tie in fp64 (5 % of that row moved in the emulation).  So a 2^40 row meets no
bias that varies along it: A has one where the bias is absent or runs along M (its own entry 0), W where it is absent or runs along N; with no bias
(m127, m300, n191, n392, k448, wide_relu, wide_gelu_tanh_nobias) both have one and meet in one element of 2^80.  Those three epilogues run where a row is wide enough for the cap to mean something (N = 1540, M = 257: interior and edge tiles
of every kernel); the narrow N edges run the exact epilogues.  Every output is finite in bf16: |y1| <= 2^80 * 1536 * 16 < 2^95.

Measured on the host (/ recomputed for the default seed by tests/test_gemm_kernel_cases.py), over CASES + PAIR_CASES at seeds {per-case default, 1, 2,
3}: the accumulation is exact in every case (acc + bias differs by at most 0.03 units of 2^-24 S0, the bias met by a 2^-40 row); the value before the
last rounding differs by at most 1.41 units of 2^-24 S (gelu_tanh; gelu_erf 1.19, silu 1.21, the fp32 gate 1.0, everything else 0).  Smallest power
of two never exceeded: 2; doubled once for the device's own order and its rcp / exp2 / exp / erf: C_NOISE = 4.  Worst moved share of any row of the
emulation: 1.3e-3 (two elements of 1540, wide_gelu_tanh and wide_silu); 0 in every case that is not one of the three activations or the fp32 gate.
Failures: 0.  On an MI355X every one of the 265 launches, the pair launches' halves and the stacked cases came back with 0 failures and 0 moved
roundings (the three activations included), every path bit for bit the one-in-flight 128^2 kernel.

Arenas.  Every operand lies in a larger allocation: GUARD_FRONT elements before it, GUARD_ROWS rows after it, pad columns where ld exceeds the width.
In A and W the pad columns [K, ld) and the guards hold NaN; so do the residual's pad columns and rows past M, and bias / gate past N (or M).  In C's
allocation everything the launch does not own holds FILL and must hold the same bits afterwards (with res == C the owned part holds the residual).
A read outside an operand that reaches an owned output shows up as NaN.  For the pair launch W2 lies BEFORE W, with n_split + GUARD_ROWS NaN rows in
front of it: the kernels' moved base W2 - n_split ldw points into memory the test owns.

Cases: 44 in CASES + 6 in PAIR_CASES; per path t128_pf1 50, t128_pf4 and t128_pf8 43 each, t192 39, t256_ph4 and t256_ph2 45 each (265 launches); 2 SEL_CASES.
"""
import functools

import numpy as np
import torch

from row_kernel_cases import FILL, GUARD_ROWS, MOVED_CAP, bf16_ulp, rbf32, rbf64

C_NOISE = 4.0
GUARD_FRONT = 64          # elements in front of every operand (a multiple of 8: the operand keeps its 16-byte alignment)
EPI = dict(bias=0, gelu_tanh=1, gate_res=2, gelu_erf=3, silu=4, relu=5)          # SVI_EPI_*
# path -> (SVI_GEMM_KERNEL, SVI_GEMM_PF)
PATHS = {"t128_pf1": (128, 1), "t128_pf4": (128, 4), "t128_pf8": (128, 8), "t192": (192, None), "t256_ph4": (259, None), "t256_ph2": (260, None)}
TILE_WIDTH = {"t128_pf1": 128, "t128_pf4": 128, "t128_pf8": 128, "t192": 192, "t256_ph4": 256, "t256_ph2": 256}
DEEP_PF = 4               # SVI_GEMM_DEEP_PF


def applies(case, path):
    """The launcher's preconditions: K % 64 == 0 for the 256-row kernels and the deep loop, K >= 4 * 64 for the deep loop, N >= 192 for the 192 tile."""
    kind, pf = PATHS[path]
    K, N = case["K"], case["N"]
    if kind != 128 and K % 64:
        return False
    if kind == 192 and N < 192:
        return False
    if pf is not None and pf > 1 and (K % 64 or K < DEEP_PF * 64):
        return False
    return True


# ------------------------------------------------------------------------------------------------ the case table
def _c(name, M=129, N=200, K=256, lda="K+8", ldw="K+64", ldc="N8+8", epi="bias", bias="n", gate=False, res=None, ldres="N8+16", stats=False,
       misalign=False, gate_f32=False, n_split=0, w_edges=True, sel_m=0, sel_n=0):
    assert (epi == "gate_res") == (res is not None) and (not gate or epi == "gate_res")
    return dict(name=name, M=M, N=N, K=K, lda=lda, ldw=ldw, ldc=ldc, epi=epi, bias=bias, gate=gate, res=res, ldres=ldres, stats=stats, misalign=misalign,
                gate_f32=gate_f32, n_split=n_split, w_edges=w_edges, sel_m=sel_m, sel_n=sel_n)


CASES = [
    # M edges (N = 200, K = 256 = exactly DEEP_PF tiles), the other axes taken in turn
    _c("m1", M=1, lda="K"),
    _c("m127", M=127, epi="gate_res", gate=True, res="own", bias=None),
    _c("m129", M=129, epi="relu", lda="2K"),
    _c("m255", M=255, epi="gate_res", res="inplace"),
    _c("m257", M=257, bias="m", ldc="2N8"),
    _c("m300", M=300, bias=None, ldw="K"),
    _c("m300_n392", M=300, N=392, epi="gate_res", gate=True, res="own"),                 # one interior 256^2 tile beside three edge tiles
    # N edges (M = 129): N % 8 != 0 tails, the idle column chunks of the 192- and 256-wide read-back
    _c("n1", N=1),
    _c("n7", N=7, epi="gate_res", gate=True, res="own"),
    _c("n9", N=9, epi="relu"),
    _c("n191", N=191, epi="gate_res", gate=True, res="inplace", bias=None),
    _c("n193", N=193, ldc="half"),
    _c("n200", N=200, epi="gate_res", res="own", ldres="ldc"),                           # gate-less residual in a buffer of its own with ldres == ldc
    _c("n257", N=257, bias="m"),
    _c("n264_misaligned", N=264, epi="gate_res", gate=True, res="own", misalign=True),    # bias / gate one element off their alignment: the scalar fetch
    _c("n392", N=392, epi="relu", bias=None),
    # K
    _c("k64", K=64, lda="K"),
    _c("k128", K=128, epi="gate_res", gate=True, res="own"),
    _c("k256", K=256, epi="gate_res", gate=True, res="inplace", ldc="N8"),
    _c("k448", K=448, epi="relu", bias=None),
    _c("k1536", K=1536, N=264, epi="gate_res", gate=True, res="own"),
    _c("k8", K=8), _c("k56", K=56, epi="gate_res", gate=True, res="own"), _c("k72", K=72, epi="relu"), _c("k136", K=136, bias="m"),      # partial K tile: the one-in-flight 128^2 kernel alone
    # strides
    _c("s_lda2k_ldwk", lda="2K", ldw="K", ldc="2N8"),
    _c("s_ldak_ldc8", lda="K", ldw="K+64", ldc="N8", M=257),
    _c("s_half_own", M=257, epi="gate_res", gate=True, res="own", ldc="half"),           # C = right half of [M, 2 N'], the left half survives
    _c("s_half_inplace", M=130, N=193, epi="gate_res", gate=True, res="inplace", ldc="half"),
    _c("s_vt", M=264, N=129, bias="m", ldc="N8+8", lda="K", ldw="K+64"),                 # the V^T launch: bias along M, ldc = L8
    # every epilogue on rows wide enough for the cap: interior and edge tiles of every kernel, an N % 8 != 0 tail
    _c("wide_bias", M=257, N=1540), _c("wide_gelu_tanh", M=257, N=1540, epi="gelu_tanh"), _c("wide_gelu_erf", M=257, N=1540, epi="gelu_erf"),
    _c("wide_silu", M=257, N=1540, epi="silu"), _c("wide_relu", M=257, N=1540, epi="relu", bias=None),
    _c("wide_gate_f32", M=257, N=1540, epi="gate_res", gate=True, gate_f32=True, res="own"),
    _c("wide_res_nogate", M=257, N=1540, epi="gate_res", res="inplace"),
    _c("wide_gelu_tanh_nobias", M=300, N=1536, epi="gelu_tanh", bias=None),
    # svi_linear_row_stats: N % 64 == 0, ldc = 2 N, ldss > M (edge rows in A only: the square of a 2^80 result is no fp32 number)
    _c("st_n64_m1", M=1, N=64, stats=True, ldc="2N8", w_edges=False), _c("st_n192", N=192, stats=True, ldc="2N8", w_edges=False),
    _c("st_n256_m300", M=300, N=256, stats=True, ldc="2N8", w_edges=False), _c("st_n512_m257", M=257, N=512, K=448, stats=True, ldc="2N8", w_edges=False),
    _c("st_k72", N=128, K=72, stats=True, ldc="2N8", w_edges=False), _c("st_bias_none", N=320, stats=True, ldc="2N8", bias=None, w_edges=False),
]
# svi_gemm_bf16_pair: ldc = N + 8; a split on the tile width of the running kernel is one launch with the moved W base, any other two launches
PAIR_CASES = [
    _c("pair_s128", N=328, n_split=128),
    _c("pair_s192", N=392, n_split=192, epi="gate_res", gate=True, res="own"),
    _c("pair_s256", M=257, N=456, n_split=256, bias="n"),
    _c("pair_s384", N=584, n_split=384, epi="gate_res", gate=True, res="inplace"),
    _c("pair_s200", N=392, n_split=200, epi="gate_res", gate=True, res="own"),          # a multiple of 8 and of no tile width: two launches on every path
    _c("pair_s72", N=264, n_split=72),
]
# the stacked pair's kernel choice (no switch set): two samples of L rows, and two projections of D columns
SEL_L, SEL_D, SEL_K = 2816, 1536, 128
SEL_CASES = [
    _c("sel_m", M=2 * SEL_L, N=SEL_D, K=SEL_K, lda="K", ldw="K", ldc="N8", sel_m=SEL_L),
    _c("sel_n", M=SEL_L, N=2 * SEL_D, K=SEL_K, lda="K", ldw="K", ldc="N8", n_split=SEL_D, sel_n=SEL_D),
]
BY_NAME = {c["name"]: c for c in CASES + PAIR_CASES + SEL_CASES}
assert len(BY_NAME) == len(CASES) + len(PAIR_CASES) + len(SEL_CASES)


def launches():
    """[(case name, path)] of the table: every case on every path whose preconditions it meets."""
    return [(c["name"], p) for c in CASES + PAIR_CASES for p in PATHS if applies(c, p)]


def dims(case):
    """The leading dimensions and C's column offset: dict(lda, ldw, ldc, c_off, ldres, ldss)."""
    M, N, K = case["M"], case["N"], case["K"]
    n8 = (N + 7) // 8 * 8
    ldc = {"N8": n8, "N8+8": n8 + 8, "2N8": 2 * n8, "half": 2 * n8}[case["ldc"]]
    return dict(lda={"K": K, "K+8": K + 8, "2K": 2 * K}[case["lda"]], ldw={"K": K, "K+64": K + 64}[case["ldw"]], ldc=ldc,
                c_off=n8 if case["ldc"] == "half" else 0, ldres=ldc if case["res"] == "inplace" or case["ldres"] == "ldc" else n8 + 16, ldss=M + 3)


def edge_rows(n):
    """{edge: index} of the rows of an operand that carry an input edge (none below 5 rows)."""
    return {"zero": 1, "tiny": 2, "huge": n - 1} if n >= 5 else {}


CANCEL_ROW = 3


# ------------------------------------------------------------------------------------------------ inputs and arenas
def _grid(rs, shape, sigma):
    """Gaussian values on the fixed-point grid 2^-3, |v| <= 4."""
    return np.clip(np.rint(8 * sigma * rs.standard_normal(shape)) / 8, -4, 4)


def _arena(block, ld, pad, rows_after=GUARD_ROWS, rows_before=0):
    """flat fp64 [GUARD_FRONT + (rows_before + rows + rows_after) ld] holding `block` [rows, width <= ld] and `pad` everywhere else; the block's offset."""
    rows, width = block.shape
    a = np.full((rows_before + rows + rows_after, ld), pad, dtype=np.float64)
    a[rows_before:rows_before + rows, :width] = block
    return np.concatenate([np.full(GUARD_FRONT, pad), a.ravel()]), GUARD_FRONT + rows_before * ld


def _vector(v, misalign):
    front = GUARD_FRONT + (1 if misalign else 0)
    return np.concatenate([np.full(front, np.nan), v, np.full(GUARD_FRONT, np.nan)]), front


def logical(case, seed=None):
    """The operands without their arenas, fp64: a [M, K], w [N, K] (a pair: W's rows, then W2's), bias [N | M] | None, gate [N] | None, res [M, N] | None."""
    M, N, K = case["M"], case["N"], case["K"]
    rs = np.random.RandomState(sum(map(ord, case["name"])) * 13 + 5 if seed is None else seed)
    a, w = _grid(rs, (M, K), 1.5), _grid(rs, (N, K), 1.5)
    scale = {"zero": 0.0, "tiny": 2.0 ** -40, "huge": 2.0 ** 40}
    bias = None if case["bias"] is None else _grid(rs, M if case["bias"] == "m" else N, 2.0)
    for edge, r in edge_rows(M).items():
        if edge == "huge" and case["bias"] == "n":
            continue          # (a 2^40 row under a bias that varies along it: see "Inputs" in the module docstring)
        a[r] *= scale[edge]
        if edge == "huge" and case["bias"] == "m":
            bias[r] = 0.0
    for edge, r in (edge_rows(N) if case["w_edges"] else {}).items():
        if edge == "huge" and case["bias"] == "m":
            continue
        w[{"tiny": 3}.get(edge, r)] *= scale[edge]          # W's tiny row is 3: row 2 of A meets an ordinary column there and a tiny one at 3
        if edge == "huge" and case["bias"] == "n":
            bias[r] = 0.0
    gate = None
    if case["gate"]:
        gate = rs.standard_normal(N).astype(np.float32).astype(np.float64) if case["gate_f32"] else _grid(rs, N, 1.0)
    res = None
    if case["res"]:
        res = _grid(rs, (M, N), 2.0)
        if M > CANCEL_ROW + 1:          # the residual nearly cancels gate y1 on one row: exactly on the even columns, to 2^-5 on the odd ones
            t = _gated(_y1(a, w, bias, case)[0][CANCEL_ROW], gate)
            res[CANCEL_ROW] = -rbf64(t * np.where(np.arange(N) % 2 == 0, 1.0, 1.0 - 2.0 ** -5))
    return a, w, bias, gate, res


def _y1(a, w, bias, case):
    acc = a @ w.T
    s0 = np.abs(a) @ np.abs(w).T
    b = 0.0 if bias is None else (bias[:, None] if case["bias"] == "m" else bias[None, :])
    return rbf64(acc + b), s0 + np.abs(b), acc + b


def _gated(y1, gate):
    return y1 if gate is None else rbf64(gate * y1)


def arenas(case, seed=None):
    """Every allocation of the launch as a flat fp64 array of bf16 values (gate: fp32 values) with the operand's element offset:
    dict(A, W, [W2], C, [bias], [bias2], [gate], [res], [ss]) of (array, offset); res == C in place: no `res` entry; W2 = (None, its offset in W's
    allocation)."""
    M, N, K, d = case["M"], case["N"], case["K"], dims(case)
    a, w, bias, gate, res = logical(case, seed)
    ns = case["n_split"]
    out = {"A": _arena(a, d["lda"], np.nan)}
    if ns:          # [n_split + GUARD_ROWS rows of NaN | W2 | GUARD_ROWS | W | GUARD_ROWS]
        w2, w2_off = _arena(w[ns:], d["ldw"], np.nan, rows_before=ns + GUARD_ROWS)
        w1, w1_off = _arena(w[:ns], d["ldw"], np.nan)
        out["W2"], out["W"] = (None, w2_off), (np.concatenate([w2, w1[GUARD_FRONT:]]), len(w2) + w1_off - GUARD_FRONT)
    else:
        out["W"] = _arena(w, d["ldw"], np.nan)
    c0 = np.full((M, N), FILL) if case["res"] != "inplace" else res
    c_arena, c_off = _arena(np.concatenate([np.full((M, d["c_off"]), FILL), c0], axis=1), d["ldc"], FILL)
    out["C"] = (c_arena, c_off + d["c_off"])
    if bias is not None:
        if ns:
            out["bias2"], out["bias"] = _vector(bias[ns:], case["misalign"]), _vector(bias[:ns], case["misalign"])
        else:
            out["bias"] = _vector(bias, case["misalign"])
    if gate is not None:
        out["gate"] = _vector(gate, case["misalign"])
    if case["res"] == "own":
        out["res"] = _arena(res, d["ldres"], np.nan)
    if case["stats"]:
        out["ss"] = _arena(np.full((N // 64, M), FILL), d["ldss"], FILL)
    return out


def owned(case):
    """Boolean mask over C's flat allocation: the elements the launch writes."""
    M, N, d = case["M"], case["N"], dims(case)
    m = np.zeros((M + GUARD_ROWS, d["ldc"]), dtype=bool)
    m[:M, d["c_off"]:d["c_off"] + N] = True
    return np.concatenate([np.zeros(GUARD_FRONT, dtype=bool), m.ravel()])


def owned_ss(case):
    m = np.zeros((case["N"] // 64 + GUARD_ROWS, dims(case)["ldss"]), dtype=bool)
    m[:case["N"] // 64, :case["M"]] = True
    return np.concatenate([np.zeros(GUARD_FRONT, dtype=bool), m.ravel()])


def c_view(case, flat):
    """The owned [M, N] block of C's flat allocation."""
    M, N, d = case["M"], case["N"], dims(case)
    return np.asarray(flat)[GUARD_FRONT:].reshape(M + GUARD_ROWS, d["ldc"])[:M, d["c_off"]:d["c_off"] + N]


def ss_view(case, flat):
    return np.asarray(flat)[GUARD_FRONT:].reshape(case["N"] // 64 + GUARD_ROWS, dims(case)["ldss"])[:case["N"] // 64, :case["M"]]


# ------------------------------------------------------------------------------------------------ fp64 reference
def _erf(v):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(v))).numpy()


def _act64(epi, y):
    with np.errstate(over="ignore"):
        if epi == "gelu_tanh":
            return 0.5 * y * (1.0 + np.tanh(0.7978845608028654 * (y + 0.044715 * y * y * y)))
        if epi == "gelu_erf":
            return 0.5 * y * (1.0 + _erf(y * 0.7071067811865476))
        if epi == "silu":
            return y / (1.0 + np.exp(-y))
        if epi == "relu":
            return np.maximum(y, 0.0)
    return y


def reference_arrays(case, a, w, bias, gate, res):
    """dict(want [M, N], s [M, N], y1, pre = acc + bias and s0 = its S0, raw = the value before the last rounding, ss = the row statistic
    [N / 64, M] | None), all fp64."""
    y1, s0, pre = _y1(a, w, bias, case)
    sy = np.maximum(s0, np.abs(y1))
    if case["epi"] == "gate_res":
        t = _gated(y1, gate)
        raw = res + t
        s = np.abs(res) + (1.0 if gate is None else np.abs(gate)) * sy
    else:
        raw, s, t = _act64(case["epi"], y1), sy, y1
    want = rbf64(raw)
    ss = (want * want).reshape(case["M"], case["N"] // 64, 64).sum(-1).T if case["stats"] else None
    return dict(want=want, s=s, y1=y1, t=t, raw=raw, ss=ss, pre=pre, s0=s0)


@functools.lru_cache(maxsize=None)
def reference(name):
    """reference_arrays of the case's own inputs, computed once and shared (read-only)."""
    case = BY_NAME[name]
    r = reference_arrays(case, *logical(case))
    for v in r.values():
        if v is not None:
            v.setflags(write=False)
    return r


def expected_c(case, want, seed=None):
    """C's flat allocation after a correct launch: what it held, with the owned block replaced."""
    flat = arenas(case, seed)["C"][0].copy()
    c_view(case, flat)[...] = want
    return flat


# ------------------------------------------------------------------------------------------------ fp32 emulation
def accumulate32(a, w):
    """a [M, K] w [N, K]^T in fp32: 64-wide K tiles (a partial last tile zero-filled), two k-steps of 32 per tile, per k-step four lane groups of 8 k
    summed one after the other, ((g0 + g1) + (g2 + g3)) added to the accumulator."""
    a, w = np.asarray(a, dtype=np.float32), np.asarray(w, dtype=np.float32)
    M, K = a.shape
    kp = -(-K // 64) * 64
    a, w = np.pad(a, ((0, 0), (0, kp - K))), np.pad(w, ((0, 0), (0, kp - K)))
    acc = np.zeros((M, w.shape[0]), dtype=np.float32)
    for k0 in range(0, kp, 32):
        parts = []
        for g in range(4):
            s = np.zeros_like(acc)
            for k in range(k0 + 8 * g, k0 + 8 * g + 8):
                s = s + a[:, k, None] * w[None, :, k]
            parts.append(s)
        acc = acc + ((parts[0] + parts[1]) + (parts[2] + parts[3]))
    return acc


def _act32(epi, y):
    y = np.asarray(y, dtype=np.float32)
    one, half = np.float32(1), np.float32(0.5)
    with np.errstate(over="ignore", invalid="ignore"):
        if epi == "gelu_tanh":          # gelu_tanh_f: x / (1 + 2^(x (x^2 A + B)))
            A = np.float32(-2.0 * 1.4426950408889634 * 0.7978845608028654 * 0.044715)
            B = np.float32(-2.0 * 1.4426950408889634 * 0.7978845608028654)
            return y / (one + np.exp2(y * (y * y * A + B)))
        if epi == "gelu_erf":
            return half * y * (one + _erf(y * np.float32(0.7071067811865476)))
        if epi == "silu":
            return y / (one + np.exp(-y))
        if epi == "relu":
            return np.maximum(y, np.float32(0))
    return y


def emulate_arrays(case, a, w, bias, gate, res, mutate=None, acc=None):
    """The launch in fp32 on the logical operands: dict(out [M, N] bf16 values in fp32, y1, raw = before the last rounding).  `mutate` plants one of
    the faults the host test must catch: "bias_transposed", "gate_after_res", "no_y1_rounding", "swap_columns".  `acc`: the fp32 accumulators of
    another kernel's loop (tests/mx8_kernel_cases.py: the MX-fp8 kernels end in the same epilogue) in place of accumulate32(a, w)."""
    M, N = case["M"], case["N"]
    f32 = lambda v: None if v is None else np.asarray(v, dtype=np.float32)
    acc = accumulate32(a, w) if acc is None else acc
    b = np.float32(0)
    if bias is not None:
        along_m = (case["bias"] == "m") != (mutate == "bias_transposed")
        idx = np.arange(M if along_m else N) % len(bias)
        b = f32(bias)[idx][:, None] if along_m else f32(bias)[idx][None, :]
    pre = acc + b
    y1 = pre if mutate == "no_y1_rounding" else rbf32(pre)
    if case["epi"] == "gate_res":
        t = y1 if gate is None else rbf32(f32(gate) * y1)
        raw = f32(res) + t
        if mutate == "gate_after_res" and gate is not None:
            raw = f32(gate) * rbf32(f32(res) + y1)
    else:
        raw, t = _act32(case["epi"], y1), y1
    out = rbf32(raw)
    if mutate == "swap_columns":
        out[:, [N // 2, N // 2 + 1]] = out[:, [N // 2 + 1, N // 2]]
    return dict(out=out, y1=y1, t=t, raw=raw, pre=pre)


def emulation(name, seed=None, mutate=None):
    case = BY_NAME[name]
    return emulate_arrays(case, *logical(case, seed), mutate=mutate)


# ------------------------------------------------------------------------------------------------ the bound
def judge(got, want, s, c=C_NOISE):
    """(moved, bad, units): elements outside the bound but within two bf16 ulps at max(|want|, s); elements further off (NaN included); the error of every
    element in units of its bound."""
    got, want, s = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(s, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - want)
        lim = 2.0 ** -8 * np.abs(want) + c * 2.0 ** -24 * s
        ok = err <= lim
        moved = ~ok & (err <= 2 * bf16_ulp(np.maximum(np.abs(want), s)))
        units = np.where(err == 0, 0.0, err / lim)
    return moved, ~ok & ~moved, units


def verdict(got, want, s, c=C_NOISE):
    """Summary of judge() over a [rows, cols] result: failures (and the first one's coordinates), the worst element error in units of the bound among the
    elements that meet it, and the worst row's share of moved roundings."""
    moved, bad, units = judge(got, want, s, c)
    share = moved.mean(axis=1)
    worst = int(np.argmax(share))
    inside = units[~moved & ~bad]
    return dict(bad=int(bad.sum()), first_bad=[int(i) for i in np.argwhere(bad)[0]] if bad.any() else None, moved=int(moved.sum()),
                worst_units=float(inside.max()) if inside.size else 0.0, worst_row=worst, worst_row_share=float(share[worst]))


def noise_units(ref, emu):
    """(accumulation, last): the fp32 noise of the emulation in units of 2^-24 S0 for acc + bias before y1's rounding, and in units of 2^-24 S for the
    value before the last rounding where both sides start from the same y1 and gate y1 (0 / 0 = 0)."""
    def units(d, s):
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(d == 0, 0.0, d / (2.0 ** -24 * s))
    same = (emu["y1"].astype(np.float64) == ref["y1"]) & (emu["t"].astype(np.float64) == ref["t"])
    acc = units(np.abs(emu["pre"].astype(np.float64) - ref["pre"]), ref["s0"])
    last = np.where(same, units(np.abs(emu["raw"].astype(np.float64) - ref["raw"]), ref["s"]), 0.0)
    return float(acc.max()), float(last.max())
