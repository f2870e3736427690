"""Case table, operands, reference, emulation and arenas of tests/test_gpu_mx8_kernels.py (no GPU imports): the MX-fp8 kernels of csrc/svi_gemm.hip —
gemm_mx8_nt_256_kernel<false> through svi_gemm_mx8 (block scales on A's rows), gemm_mx8_nt_256_kernel<true> through svi_gemm_mx8_wscaled (block scales on
W's rows) and mx8_quantize_kernel through svi_mx8_quantize — in the strided forms the DiT launches.  tests/test_mx8_kernel_cases.py runs all of it on
the host.  The bound (judge / verdict, C_NOISE, MOVED_CAP), the epilogue references and the fp32 epilogue are those of tests/gemm_kernel_cases.py: the MX
kernels end in the same gemm256_epilogue.

operands    The GEMM tests build e4m3 bytes and the scale table themselves.  Body bytes hold clip(round(2 g), -6, 6) / 2 for Gaussian g: multiples of
            2^-1, at most 3 in magnitude, every one an e4m3 value.  Scale codes are 127 + e with e drawn per row and per 32-block from -3 .. 3, so
            adjacent blocks and adjacent rows differ almost everywhere (6 in 7): a block or a row taking its neighbour's scale shows.  Every product and
            every partial sum is then a multiple of 2^-5 below 2^24 2^-5: fp32 accumulation is exact IN ANY ORDER, and the module asserts
            S0 / grid < 2^22 for every case it builds (exactness(): 14.7 bits at K = 128, 15.3 at 256, 16.9 at 1536, 19.0 at K = 8960).  Biases, residuals
            and bf16-valued gates lie on gemm_kernel_cases._grid (2^-3, |v| <= 4), so acc + bias, gate y1 and res + ... are exact too and only the result's one
            bf16 rounding remains, the same in fp32 and fp64.  Edge rows of the SCALED operand (gemm_kernel_cases.edge_rows): one whose every scale
            code is shifted by +40, one by -40, one of zeros (bytes 0x00 and 0x80 mixed); the unit-scale operand has a zero row.  A 2^40 row meets no bias
            that varies along it (the reason: gemm_kernel_cases, "Inputs"): A's under svi_gemm_mx8 only where the bias is absent, W's under
            svi_gemm_mx8_wscaled where it is absent or runs along N (its own entry 0).
not exact   the fp32 gelu_tanh / gelu_erf / silu, an fp32 gate, a bias added to a 2^-40 row: the bound |got - want| <= 2^-8 |want| + C_NOISE 2^-24 S and
            the cap on moved roundings (MOVED_CAP of any row) apply unchanged, S from the dequantised operands as gemm_kernel_cases defines it.  Those
            epilogues run where a row is wide (N = 1540); the narrow N edges run the exact ones.
tables      M = N = K = 256, one tile, no sum at all: one operand is the identity (byte 0x38 = 1.0), the other holds every finite e4m3 code
            (test_gpu_gemm_w8.byte_table).  With the table in the unit-scale operand (scale codes 127) C is the widened byte: decoding.  With the table in
            the scaled operand and codes 127 + ((5 r + 11 b) % 121 - 60) for row r and block b, C[r-th row or column] = widen(byte) 2^(code - 127), a
            normal bf16 number throughout: it pins dword [kt][r], byte b and the lane-half selection for every row and block of a tile.
arenas      Every operand lies in a larger allocation.  A8 / W8: guard bytes in front, GUARD_ROWS rows after, pad columns [K, ld), all 0x7F (NaN);
            bias / gate / residual: NaN around them.  The scale table [K / 128][sc_rows], sc_rows = ceil256(rows) or that + 256, holds 0xFF (NaN) in every
            row past the operand's and in a slab of sc_rows dwords before and after: the kernel fetches whole 256-row slabs, and nothing owned may become
            NaN from them.  C's allocation holds FILL wherever the launch does not own it.
emulation   the same arithmetic in fp32 with the K tile (128) taken as two 64-steps of two 32-blocks: the block's sum of raw e4m3 products first, scaled,
            then added — another order than the reference's.  It stands for correct fp32 in another order and is not claimed bit-equal to the device.
            `mutate` plants the faults the host test must catch (MUTATIONS).

Measured on the host (tests/test_mx8_kernel_cases.py): reference and emulation agree to the bit in every case whose epilogue is exact.  Noise in units
of 2^-24 S: the accumulation 0 (a bias met by the 2^-40 row: up to 0.07, below every rounding); the last step at most 1.41 (gelu_tanh; silu 1.21,
gelu_erf 1.19), within the C_NOISE / 2 that file measured; the fp32 gate's product moves 3 roundings of 395780, at most one in a row: the worst moved
share of a row is 6.5e-4 (one element of 1540), and 0 outside the three activations and the fp32 gate.
On an MI355X (profiles/mx8_kernels_parity.txt): 0 failures; every launch whose epilogue is exact came back with the reference's bits, the eight
accumulation-only cases included — the scaled matrix instruction added the on-grid products exactly, K = 128 .. 8960; 3 moved roundings, the fp32 gate's.
Cases: 36 in CASES + 14 in WSC_CASES + 4 TABLE_CASES + SEAM.
"""
import functools

import numpy as np
import torch

import gemm_kernel_cases as gk
from gemm_kernel_cases import C_NOISE, EPI, GUARD_FRONT, judge, noise_units, verdict          # noqa: F401  (the bound is that file's)
from row_kernel_cases import FILL, GUARD_ROWS, MOVED_CAP, rbf32, rbf64                        # noqa: F401
from test_gpu_gemm_w8 import FINITE, byte_table

BLOCK, KTILE, TILE = 32, 128, 256
NAN8 = 0x7F
DECODE = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().double().numpy()          # byte -> value (0x7F, 0xFF: NaN)
_GRID_BYTES = np.array([int(np.flatnonzero(DECODE == v / 2)[0]) for v in range(-6, 7)], dtype=np.uint8)     # -3 .. 3 in steps of 1/2 (0 -> 0x00)
SHIFT = {"zero": 0, "tiny": -40, "huge": 40}
MUTATIONS = ("scale_bytes_reversed", "scale_blocks_swapped", "scale_row_plus_one", "drop_last_k_tile", "dup_last_row", "read_a_pad", "write_c_pad")


# ------------------------------------------------------------------------------------------------ the case table
def _c(name, M=129, N=200, K=256, lda="K+16", ldw="K+64", ldc="N8+8", epi="bias", bias="n", gate=False, res=None, ldres="N8+16", gate_f32=False,
       misalign=False, wsc=False, sc_extra=0, a_front=GUARD_FRONT, special=None):
    assert (epi == "gate_res") == (res is not None) and (not gate or epi == "gate_res") and (wsc or bias != "m") and (not wsc or epi == "bias")
    return dict(name=name, M=M, N=N, K=K, lda=lda, ldw=ldw, ldc=ldc, epi=epi, bias=bias, gate=gate, res=res, ldres=ldres, gate_f32=gate_f32, misalign=misalign,
                wsc=wsc, sc_extra=sc_extra, a_front=a_front, special=special, stats=False)


CASES = [          # svi_gemm_mx8: one 256 x 256 x 128 tile, two stages
    # M edges: the clamped source rows, stale scale rows in the last slab
    _c("m1", M=1, lda="K"),
    _c("m255", M=255, epi="gate_res", res="inplace", sc_extra=256),
    _c("m256", M=256, bias=None),
    _c("m257", M=257, ldc="half"),
    _c("m300", M=300, bias=None, ldw="K", sc_extra=256),
    _c("m513", M=513),                                                                     # three row panels: group height 2, a last group of one
    # N edges
    _c("n1", N=1),
    _c("n7", N=7, epi="gate_res", gate=True, res="own"),
    _c("n9", N=9, epi="relu", sc_extra=256),
    _c("n256", N=256, M=300, ldc="N8"),
    _c("n257", N=257, bias=None),
    _c("n264_misaligned", N=264, epi="gate_res", gate=True, res="own", misalign=True),      # bias / gate one element off their alignment: the scalar fetch
    _c("n520_m513", M=513, N=520, sc_extra=256),                                           # 9 tiles: one XCD band of two
    _c("n1100_m300", M=300, N=1100, bias=None),                                            # 10 tiles: two XCD bands of two
    # K: nk = 1, 2, 3 (odd), 12, 70
    _c("k128", K=128, epi="gate_res", gate=True, res="own"),
    _c("k384", K=384, epi="relu", bias=None),
    _c("k1536", K=1536, N=264, epi="gate_res", gate=True, res="own", sc_extra=256),
    _c("k8960_ffn2", M=300, N=264, K=8960, epi="gate_res", gate=True, res="inplace"),      # the ffn2 launch: the gated residual written in place
    # strides
    _c("s_lda2k_ldwk", lda="2K", ldw="K", ldc="N8"),
    _c("s_ldak_ldc8", M=257, lda="K", ldc="N8"),
    _c("s_half_own", M=257, epi="gate_res", gate=True, res="own", ldc="half"),             # the q | k form: C = right half of [M, 2 N8], the left survives
    _c("s_half_inplace", M=130, N=193, epi="gate_res", gate=True, res="inplace", ldc="half"),
    _c("s_a_16_not_32", M=257, a_front=GUARD_FRONT + 16),                                  # A8 on a base that is 16- but not 32-byte aligned
    # every epilogue on rows wide enough for the cap, interior and edge tiles
    _c("wide_bias", M=257, N=1540), _c("wide_gelu_tanh", M=257, N=1540, epi="gelu_tanh"), _c("wide_gelu_erf", M=257, N=1540, epi="gelu_erf"),
    _c("wide_silu", M=257, N=1540, epi="silu", sc_extra=256), _c("wide_relu", M=257, N=1540, epi="relu", bias=None),
    _c("wide_gate_bf16", M=257, N=1540, epi="gate_res", gate=True, res="own"),
    _c("wide_gate_f32", M=257, N=1540, epi="gate_res", gate=True, gate_f32=True, res="own"),
    _c("wide_res_nogate", M=257, N=1540, epi="gate_res", res="inplace"),
    _c("wide_res_nogate_own", M=257, N=1540, epi="gate_res", res="own", bias=None),
    _c("wide_gelu_tanh_nobias", M=300, N=1536, epi="gelu_tanh", bias=None),
    _c("wide_gate_inplace", M=300, N=1536, epi="gate_res", gate=True, res="inplace", ldc="N8"),
    # 6 x 16 tiles: tn >= 16 takes group height 5, a last group of one
    _c("tn16_m1300", M=1300, N=4096, K=128, lda="K", ldw="K", ldc="N8"),
    _c("tn16_m1300_nobias", M=1300, N=4096, K=128, bias=None, lda="2K", sc_extra=256),
]
WSC_CASES = [          # svi_gemm_mx8_wscaled: scales on W's rows, the plain bias epilogue, ldc = N8 + 8
    _c("w_m1", M=1, N=300, bias="n", wsc=True),
    _c("w_m256", M=256, N=300, bias="m", wsc=True),
    _c("w_m257", M=257, N=300, bias=None, wsc=True, sc_extra=256),
    _c("w_m300", M=300, N=300, bias="m", wsc=True),
    _c("w_n1", M=257, N=1, bias="m", wsc=True),
    _c("w_n255", M=257, N=255, bias="n", wsc=True),
    _c("w_n257", M=257, N=257, bias=None, wsc=True),
    _c("w_n520", M=300, N=520, bias="m", wsc=True, sc_extra=256),
    _c("w_n520_bias_n", M=300, N=520, bias="n", wsc=True),
    _c("w_k128", M=300, N=300, K=128, bias="m", wsc=True),
    _c("w_k384", M=257, N=300, K=384, bias=None, wsc=True),
    _c("w_k1536", M=257, N=300, K=1536, bias="m", wsc=True, sc_extra=256),
    _c("w_k1536_bias_n", M=256, N=257, K=1536, bias="n", wsc=True),
    _c("w_vt", M=512, N=297, bias="m", wsc=True, lda="K", ldw="K"),                         # the V^T launch: 512 channels x 297 tokens, bias along M
]
TABLE_CASES = [          # identity against every finite byte: decoding (table in the unit-scale operand) and scale layout (table in the scaled operand)
    _c("table_unit", M=256, N=256, bias=None, special="table_unit"), _c("table_scaled", M=256, N=256, bias=None, special="table_scaled"),
    _c("w_table_unit", M=256, N=256, bias=None, wsc=True, special="table_unit"), _c("w_table_scaled", M=256, N=256, bias=None, wsc=True, special="table_scaled"),
]
SEAM = _c("seam_quantised", M=300, N=264, K=384, special="seam", sc_extra=256)          # A8 and its scales come from the quantiser (the oracle's here)
NAN_CASES = ("m300", "w_m300")          # a 0x7F byte planted at NAN_AT (row, k) of A8 (second row panel, second K tile), a 0xFF byte at NAN_AT_W of W8
NAN_AT, NAN_AT_W = (257, 130), (131, 200)
GM_CASE, GM_VALUES = "m513", (1, 3)          # the launcher's group-height switch on three row panels
BY_NAME = {c["name"]: c for c in CASES + WSC_CASES + TABLE_CASES + [SEAM]}
assert len(BY_NAME) == len(CASES) + len(WSC_CASES) + len(TABLE_CASES) + 1


def ceil256(n):
    return (n + TILE - 1) // TILE * TILE


def dims(case):
    """The leading dimensions (A8 / W8: bytes), C's column offset and the scale table's row count."""
    M, N, K = case["M"], case["N"], case["K"]
    n8 = (N + 7) // 8 * 8
    ldc = {"N8": n8, "N8+8": n8 + 8, "half": 2 * n8}[case["ldc"]]
    return dict(lda={"K": K, "K+16": K + 16, "2K": 2 * K}[case["lda"]], ldw={"K": K, "K+64": K + 64}[case["ldw"]], ldc=ldc,
                c_off=n8 if case["ldc"] == "half" else 0, ldres=ldc if case["res"] == "inplace" or case["ldres"] == "ldc" else n8 + 16,
                sc_rows=ceil256(N if case["wsc"] else M) + case["sc_extra"])


def accumulation_only(case):
    """No bias, no activation, no residual: what comes back is the accumulator's one rounding."""
    return case["epi"] == "bias" and case["bias"] is None


def exact_epilogue(case):
    """Every step after the accumulation is exact in fp32 on the grid operands (a bias met by the 2^-40 row aside)."""
    return case["epi"] in ("bias", "relu") or (case["epi"] == "gate_res" and not case["gate_f32"])


# ------------------------------------------------------------------------------------------------ operands
def dequantise(q8, codes):
    """bytes [R, K], E8M0 codes [R, K / 32] | None (unit scales) -> fp64 values."""
    v = DECODE[q8]
    return v if codes is None else v * np.repeat(np.ldexp(1.0, codes.astype(np.int64) - 127), BLOCK, axis=1)


def _table_operands(case):
    eye = np.zeros((TILE, TILE), dtype=np.uint8)
    eye[np.arange(TILE), np.arange(TILE)] = 0x38
    table = byte_table(TILE, TILE).numpy()
    if case["special"] == "table_scaled":
        r, b = np.arange(TILE)[:, None], np.arange(TILE // BLOCK)[None, :]
        scaled, unit, codes = table, eye, (127 + ((5 * r + 11 * b) % 121 - 60)).astype(np.uint8)
    else:
        scaled, unit, codes = eye, table, np.full((TILE, TILE // BLOCK), 127, dtype=np.uint8)
    return scaled, unit, codes


def logical(case, seed=None):
    """The operands without their arenas: dict(a8 [M, K] u8, w8 [N, K] u8, codes [rows of the scaled operand, K / 32] u8, shift [those rows] (the power of
    two an edge row's codes are moved by), a, w (fp64, dequantised), bias, gate, res (fp64 | None), x (the seam case's bf16 activation))."""
    M, N, K, wsc = case["M"], case["N"], case["K"], case["wsc"]
    S, U = (N, M) if wsc else (M, N)
    rs = np.random.RandomState(sum(map(ord, case["name"])) * 17 + 3 if seed is None else seed)
    shift, x = np.zeros(S, dtype=np.int64), None
    if case["special"] in ("table_unit", "table_scaled"):
        scaled, unit, codes = _table_operands(case)
    else:
        body = lambda n: _GRID_BYTES[(np.clip(np.rint(2 * rs.standard_normal((n, K))), -6, 6) + 6).astype(np.int64)]
        scaled, unit = body(S), body(U)
        codes = 127 + rs.randint(-3, 4, size=(S, K // BLOCK))
        bias_varies_along_scaled_row = case["bias"] == ("m" if wsc else "n")
        for edge, r in gk.edge_rows(S).items():
            if edge == "huge" and bias_varies_along_scaled_row:
                continue
            shift[r] = SHIFT[edge]
            codes[r] = codes[r] + SHIFT[edge]
            if edge == "zero":
                scaled[r] = np.where(rs.rand(K) < 0.5, 0x00, 0x80)
        if U >= 5:
            unit[1] = np.where(rs.rand(K) < 0.5, 0x00, 0x80)
        if case["special"] == "seam":          # an on-grid bf16 activation through the quantiser: its bytes and codes are the oracle's
            from oracle import mx8_oracle as mx
            x = gk._grid(rs, (M, K), 1.5) * np.ldexp(1.0, rs.randint(-3, 4, size=(M, 1)))
            q, e = mx.mx8_quantize(torch.from_numpy(x).float())
            scaled, codes, shift = q.view(torch.uint8).numpy().copy(), e.numpy().copy(), np.zeros(S, dtype=np.int64)
    codes = codes.astype(np.uint8)
    a8, w8 = (unit, scaled) if wsc else (scaled, unit)
    a, w = (dequantise(a8, None), dequantise(w8, codes)) if wsc else (dequantise(a8, codes), dequantise(w8, None))
    bias = None if case["bias"] is None else gk._grid(rs, M if case["bias"] == "m" else N, 2.0)
    if bias is not None and wsc and case["bias"] == "n" and "huge" in gk.edge_rows(S):
        bias[gk.edge_rows(S)["huge"]] = 0.0
    gate = None
    if case["gate"]:
        gate = rs.standard_normal(N).astype(np.float32).astype(np.float64) if case["gate_f32"] else gk._grid(rs, N, 1.0)
    res = None
    if case["res"]:
        res = gk._grid(rs, (M, N), 2.0)
        if M > gk.CANCEL_ROW + 1:          # the residual nearly cancels gate y1 on one row, as in the bf16 cases
            t = gk._gated(gk._y1(a[gk.CANCEL_ROW:gk.CANCEL_ROW + 1], w, bias, case)[0][0], gate)
            res[gk.CANCEL_ROW] = -rbf64(t * np.where(np.arange(N) % 2 == 0, 1.0, 1.0 - 2.0 ** -5))
    return dict(a8=a8, w8=w8, codes=codes, shift=shift, a=a, w=w, bias=bias, gate=gate, res=res, x=x)


@functools.lru_cache(maxsize=None)
def operands(name):
    """logical() of the case's own seed, once (read-only)."""
    ops = logical(BY_NAME[name])
    for v in ops.values():
        if v is not None:
            v.setflags(write=False)
    return ops


def pack_scales(codes, sc_rows, fill=0xFFFFFFFF):
    """codes [R, K / 32] -> the device table uint32 [K / 128][sc_rows]: byte b of dword [kt][r] = block 4 kt + b of row r; rows past R hold `fill`."""
    R, nb = codes.shape
    t = codes.astype(np.uint32).reshape(R, nb // 4, 4)
    tab = np.full((nb // 4, sc_rows), fill, dtype=np.uint32)
    tab[:, :R] = (t[..., 0] | (t[..., 1] << 8) | (t[..., 2] << 16) | (t[..., 3] << 24)).T
    return tab


def _byte_arena(block, ld, front):
    rows, width = block.shape
    a = np.full((rows + GUARD_ROWS, ld), NAN8, dtype=np.uint8)
    a[:rows, :width] = block
    return np.concatenate([np.full(front, NAN8, dtype=np.uint8), a.ravel()]), front


def arenas(case, ops=None):
    """Every allocation of the launch with the operand's element offset: A8, W8 (uint8), SC (uint32), C, [bias], [res] (fp64 holding bf16 values),
    [gate] (fp64 holding fp32 values); res == C in place: no `res` entry."""
    M, N, d = case["M"], case["N"], dims(case)
    ops = operands(case["name"]) if ops is None else ops
    guard = np.full(d["sc_rows"], 0xFFFFFFFF, dtype=np.uint32)
    out = {"A8": _byte_arena(ops["a8"], d["lda"], case["a_front"]), "W8": _byte_arena(ops["w8"], d["ldw"], GUARD_FRONT),
           "SC": (np.concatenate([guard, pack_scales(ops["codes"], d["sc_rows"]).ravel(), guard]), d["sc_rows"])}
    c0 = np.full((M, N), FILL) if case["res"] != "inplace" else ops["res"]
    c_arena, c_off = gk._arena(np.concatenate([np.full((M, d["c_off"]), FILL), c0], axis=1), d["ldc"], FILL)
    out["C"] = (c_arena, c_off + d["c_off"])
    if ops["bias"] is not None:
        out["bias"] = gk._vector(ops["bias"], case["misalign"])
    if ops["gate"] is not None:
        out["gate"] = gk._vector(ops["gate"], case["misalign"])
    if case["res"] == "own":
        out["res"] = gk._arena(ops["res"], d["ldres"], np.nan)
    return out


def owned(case):
    """Boolean mask over C's flat allocation: the elements the launch writes."""
    M, N, d = case["M"], case["N"], dims(case)
    m = np.zeros((M + GUARD_ROWS, d["ldc"]), dtype=bool)
    m[:M, d["c_off"]:d["c_off"] + N] = True
    return np.concatenate([np.zeros(GUARD_FRONT, dtype=bool), m.ravel()])


def c_view(case, flat):
    """The owned [M, N] block of C's flat allocation."""
    M, N, d = case["M"], case["N"], dims(case)
    return np.asarray(flat)[GUARD_FRONT:].reshape(M + GUARD_ROWS, d["ldc"])[:M, d["c_off"]:d["c_off"] + N]


def expected_c(case, want):
    """C's flat allocation after a correct launch: what it held, with the owned block replaced."""
    flat = arenas(case)["C"][0].copy()
    c_view(case, flat)[...] = want
    return flat


# ------------------------------------------------------------------------------------------------ fp64 reference
def reference_of(case, ops):
    """gemm_kernel_cases.reference_arrays on the dequantised operands: dict(want, s, y1, t, raw, pre, s0, ss = None)."""
    return gk.reference_arrays(case, ops["a"], ops["w"], ops["bias"], ops["gate"], ops["res"])


@functools.lru_cache(maxsize=None)
def reference(name):
    """reference_of the case's own operands, computed once and shared (read-only); the grid assertion is made here."""
    case = BY_NAME[name]
    r = reference_of(case, operands(name))
    for v in r.values():
        if v is not None:
            v.setflags(write=False)
    if case["special"] not in ("table_unit", "table_scaled"):
        assert exactness(name, r) < 22.0, name
    return r


def exactness(name, ref=None):
    """log2 of max S0 / grid over the products alone: the bits the largest partial sum can need (grid = 2^-5 times the scaled row's own shift; the seam
    case's activation lies on 2^-3 times its row's power of two, at least 2^-3: the products on 2^-7)."""
    case, ops = BY_NAME[name], operands(name)
    ref = reference(name) if ref is None else ref
    b = 0.0 if ops["bias"] is None else np.abs(ops["bias"][:, None] if case["bias"] == "m" else ops["bias"][None, :])
    grid = np.ldexp(1.0, ops["shift"] - (7 if case["special"] == "seam" else 5))
    s0 = (ref["s0"] - b) / (grid[None, :] if case["wsc"] else grid[:, None])
    assert np.array_equal(s0, np.rint(s0))          # (S0 itself lies on the grid)
    return float(np.log2(max(s0.max(), 1.0)))


# ------------------------------------------------------------------------------------------------ fp32 emulation
def accumulate_mx(a8, w8, codes, wsc, mutate=None):
    """fp32 accumulators [M, N] of the MX loop: per 128-wide K tile two 64-steps of two 32-blocks; a block's raw e4m3 products are summed, the sum is
    scaled by the block's 2^(code - 127) (code 0xFF: NaN) and added.  a8 / w8: bytes [rows, K] (a8 may come from an arena read: see emulate)."""
    av, wv = DECODE[a8].astype(np.float32), DECODE[w8].astype(np.float32)
    with np.errstate(over="ignore"):
        sc = np.where(codes == 0xFF, np.nan, np.ldexp(1.0, codes.astype(np.int64) - 127)).astype(np.float32)
    acc = np.zeros((av.shape[0], wv.shape[0]), dtype=np.float32)
    nk = a8.shape[1] // KTILE - (1 if mutate == "drop_last_k_tile" else 0)
    for kt in range(nk):
        for s in range(2):
            for h in range(2):
                b = 4 * kt + 2 * s + h
                sb = {"scale_bytes_reversed": 4 * kt + 3 - (2 * s + h), "scale_blocks_swapped": 4 * kt + 2 * s + (1 - h)}.get(mutate, b)
                col = sc[:, sb]
                if mutate == "scale_row_plus_one":
                    col = np.append(col[1:], np.float32(np.nan))          # (the last row finds the stale 0xFF of the row past the operand)
                with np.errstate(invalid="ignore"):
                    part = av[:, BLOCK * b:BLOCK * (b + 1)] @ wv[:, BLOCK * b:BLOCK * (b + 1)].T
                    acc = acc + part * (col[None, :] if wsc else col[:, None])
    return acc


def emulate(name, mutate=None):
    """The launch in fp32 from the case's ARENAS: dict(out [M, N], y1, t, raw, pre, c = C's flat allocation afterwards)."""
    assert mutate is None or mutate in MUTATIONS
    case, ops, d = BY_NAME[name], operands(name), dims(BY_NAME[name])
    M, N, K = case["M"], case["N"], case["K"]
    flat, off = arenas(case)["A8"]
    cols = np.arange(K)
    if mutate == "read_a_pad":
        cols[K - 1] = K          # the first pad column (lda == K: the next row's first byte, the guard after the last row)
    a8 = flat[off + np.arange(M)[:, None] * d["lda"] + cols[None, :]]
    acc = accumulate_mx(a8, ops["w8"], ops["codes"], case["wsc"], mutate)
    with np.errstate(invalid="ignore", over="ignore"):
        e = gk.emulate_arrays(case, ops["a"], ops["w"], ops["bias"], ops["gate"], ops["res"], acc=acc)
    if mutate == "dup_last_row" and M >= 2:
        e["out"][M - 2] = e["out"][M - 1]
    e["c"] = expected_c(case, e["out"].astype(np.float64))
    if mutate == "write_c_pad":
        e["c"][arenas(case)["C"][1] + N] = 1.0          # the element right of row 0's last owned one
    return e


# ------------------------------------------------------------------------------------------------ the quantiser's inputs
QUANT_SHAPES = ((1, 128), (37, 256), (257, 1536))
_TIES = (480.0, -496.0, 17.0, 19.0, -21.0, -23.0, 27.0, 29.0,                                       # the block maximum (-> scale 2^0) and a value beside it saturate;
         1.5 * 2.0 ** -9, 0.5 * 2.0 ** -9, 2.5 * 2.0 ** -9, -3.5 * 2.0 ** -9, 2.0 ** -10 * 0.75)     # halfway between two codes, both parities, normal and subnormal


def quant_input(rows, K, seed=7):
    """x [rows, K] fp64 holding bf16 values: Gaussian rows over eight decades with, in row 0 (and in the last row's last four blocks): a block of exact
    e4m3 ties in both parities beside values that saturate; a block with +inf and -inf; an all-zero block; a block of bf16 subnormals."""
    rs = np.random.RandomState(seed + rows + K)
    x = rbf64(rs.standard_normal((rows, K)) * np.logspace(-5, 3, rows)[:, None])
    spots = [(0, 0)] + ([(rows - 1, K - 4 * BLOCK)] if rows > 2 else [])
    for r, c in spots:
        x[r, c:c + 4 * BLOCK] = rbf64(rs.standard_normal(4 * BLOCK))
        x[r, c:c + len(_TIES)] = _TIES
        x[r, c + BLOCK + 3], x[r, c + BLOCK + 20] = np.inf, -np.inf
        x[r, c + 2 * BLOCK:c + 3 * BLOCK] = 0.0
        x[r, c + 3 * BLOCK:c + 4 * BLOCK] = rs.randint(-127, 128, size=BLOCK) * 2.0 ** -133
    assert np.array_equal(np.where(np.isfinite(x), rbf64(np.where(np.isfinite(x), x, 0.0)), x), x)
    return x


def quant_nan_places(rows, K):
    """(row, column) of the NaNs planted into quant_input: in the tie block, in the all-zero block, at a row's last element, in an ordinary block."""
    return sorted({(0, 5), (0, 2 * BLOCK + 9), (rows - 1, K - 1 - 3 * BLOCK), (rows // 2, K // 2 + 1)})
