"""Case tables, references and the per-element bound of tests/test_gpu_row_kernels.py (no GPU imports): the row kernels of
csrc/svi_elementwise.hip — RMSNorm (+ RoPE) through svi_rmsnorm_rope_qk, the launch the DiT block makes on its q | k buffer, and
LayerNorm (+ affine | + modulate) through svi_layernorm_modulate.  tests/test_row_kernel_cases.py runs all of it on the host.

Per operation there are three functions:

reference   fp64 arithmetic, rounded to bf16 only where the kernels write rbf() or cast their result (rbf64 rounds fp64 -> bf16 in ONE step):
              RMSNorm    rbf(rbf(x rs) g), rs = (mean x^2 + eps)^-1/2        wan_dit_oracle.rms_norm_full
              + RoPE     rbf((a c - b s) out_scale), rbf((a s + b c) out_scale) per pair, (c, s) the fp64 table stored as fp32
                         (wan_dit_oracle.rope_table_3d), the scale before the only rounding; without RoPE rbf(y out_scale)
              LayerNorm  rbf((x - mean) rstd [w + b]), then rbf(rbf(y rbf(1 + scale)) + shift)    wan_dit_oracle.layer_norm / modulated_norm
emulation   the same in fp32 in the kernels' order: a lane's partial sum over its 8-element chunks (chunk = lane + 64 c), a 64-lane xor tree,
            one division, one reciprocal square root.  It is not held to be bit-exact with the device (its rsqrt and division are the device's own): it exists
            to measure on the host how often a last-bit difference of the fp32 statistic moves a bf16 rounding.
bound       per element |got - want| <= 2^-8 |want| + 2^-20 s: one bf16 half-ulp plus fp32 noise; s = (|a| + |b|) out_scale for a rotated pair
            (a rotation can cancel: its noise is relative to its inputs), |want| otherwise.  Both sides are bf16 values, one ulp is more than
            2^-8 |want|, so outside a cancelling pair this admits equality and nothing else.  An element that misses it is a MOVED ROUNDING if it lies within two bf16 ulps, and a
            failure otherwise, however rare; moved roundings may be at most MOVED_CAP of the elements of ANY row (the cap
            test_cross_attention_normalises_q_as_it_reads_it uses for the same effect).

The two-ulp window of a moved rounding is taken at max(|want|, s), as the noise term is: in a rotated pair an intermediate rounding that moves
shifts a or b by one of ITS ulps, and where the rotation cancels that is many ulps of the small result.  Taken at |want| alone the window fails
the fp32 emulation itself, which is correct arithmetic by construction: 3 elements of 1.1e7 over six other seeds of the RMSNorm table (all in
cancelling pairs), none of 7.7e6 for LayerNorm, where s = |want| and the two coincide.
"""
import functools

import numpy as np
import torch

from oracle import wan_dit_oracle as wdo

EPS = 1e-6
QK_SCALE = float(np.float32(0.12751743))          # SVI_QK_SCALE_LOG2E (csrc/svi_common.h): softmax_scale * log2(e) for head_dim 128
MOVED_CAP = 2e-3
ROW_COUNTS = (1, 3, 4, 5, 15, 16, 17, 33)         # first / last row of a wave's 4-row walk and of a workgroup's 16 rows, a lone row in a last workgroup
MULTI_ROW_DIMS = (1536, 5120)                     # rmsnorm_rope_rows_kernel / ln_mod_rows_kernel <3 | 10, 4, ...>
GUARD_ROWS = 3                                    # rows allocated past `rows`, which no launch may touch
SCALES = {"11": (1.0, 1.0), "q1": (QK_SCALE, 1.0), "qh": (QK_SCALE, 0.5)}
ROPE_NONE, ROPE_AXIS, ROPE_TOKEN = 0, 1, 2
GRID_A, GRID_B = (2, 3, 5), (3, 4, 6)             # f > 1 and h != w: an h / w swap or a wrong h w divisor moves the table row


# ------------------------------------------------------------------------------------------------ number formats
def rbf64(v):
    """fp64 -> the nearest bf16 value (ties to even) in one rounding, returned as fp64."""
    v = np.asarray(v, dtype=np.float64)
    _, e = np.frexp(v)
    q = np.ldexp(1.0, e - 8)
    return np.rint(v / q) * q


def rbf32(v):
    """fp32 -> bf16 -> fp32 (ties to even), as the device's cast."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def bf16_ulp(v):
    """Spacing of bf16 at |v| (0 at 0)."""
    v = np.abs(np.asarray(v, dtype=np.float64))
    _, e = np.frexp(v)
    return np.where(v > 0, np.ldexp(1.0, e - 8), 0.0)


def _rnd_t(t):
    return torch.from_numpy(rbf64(t.numpy()))


# ------------------------------------------------------------------------------------------------ the bound
def judge(got, want, s=None):
    """(moved, bad): boolean arrays — elements outside the bound but within two bf16 ulps at max(|want|, s), and elements further off.  s = None: |want|."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    s = np.abs(want) if s is None else np.asarray(s, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want)
        ok = err <= 2.0 ** -8 * np.abs(want) + 2.0 ** -20 * s
        moved = ~ok & (err <= 2 * bf16_ulp(np.maximum(np.abs(want), s)))
    return moved, ~ok & ~moved


def verdict(got, want, s=None):
    """Summary of judge() over a [rows, cols] result: failures, and the worst row's share of moved roundings."""
    moved, bad = judge(got, want, s)
    share = moved.reshape(moved.shape[0], -1).mean(axis=1)
    worst = int(np.argmax(share))
    return dict(bad=int(bad.sum()), first_bad=[int(i) for i in np.argwhere(bad)[0]] if bad.any() else None, moved=int(moved.sum()),
                share=float(moved.mean()), worst_row=worst, worst_row_share=float(share[worst]))


# ------------------------------------------------------------------------------------------------ RMSNorm + RoPE cases
def _rms(name, dim, rows, nop, ld, rope, grid=GRID_B, row0=0, period=0, scales="q1"):
    return dict(name=name, dim=dim, rows=rows, nop=nop, ld=ld, rope=rope, grid=grid, row0=row0, period=period, scales=scales)


def _walk(dim, tag):
    """Every row count at one width on the per-token table, the other axes taken in turn."""
    return [
        _rms(f"{tag}_r1", dim, 1, 2, "2dim", ROPE_TOKEN, GRID_A, 7, 0, "q1"),
        _rms(f"{tag}_r3", dim, 3, 2, "2dim+64", ROPE_TOKEN, GRID_B, 0, 1, "qh"),          # period = rows / 3
        _rms(f"{tag}_r4", dim, 4, 1, "dim", ROPE_TOKEN, GRID_A, 7, 2, "11"),              # period = rows / 2
        _rms(f"{tag}_r5", dim, 5, 2, "2dim", ROPE_TOKEN, GRID_B, 0, 0, "q1"),
        _rms(f"{tag}_r15", dim, 15, 2, "2dim+64", ROPE_TOKEN, GRID_A, 7, 5, "qh"),
        _rms(f"{tag}_r16", dim, 16, 2, "2dim", ROPE_TOKEN, GRID_B, 7, 8, "q1"),
        _rms(f"{tag}_r17", dim, 17, 1, "2dim", ROPE_TOKEN, GRID_A, 7, 0, "q1"),           # one operand in a two-operand row: the other half stays
        _rms(f"{tag}_r33", dim, 33, 2, "2dim+64", ROPE_TOKEN, GRID_B, 7, 11, "q1"),
        _rms(f"{tag}_r17_norope", dim, 17, 2, "2dim+64", ROPE_NONE, scales="qh"),
        _rms(f"{tag}_r5_norope", dim, 5, 1, "dim", ROPE_NONE, scales="11"),
        _rms(f"{tag}_r17_axis", dim, 17, 2, "2dim", ROPE_AXIS, GRID_B, 7, 0, "q1"),       # axis tables: the generic kernel at this width
    ]


RMS_CASES = _walk(1536, "w1536") + _walk(5120, "w5120") + [
    _rms("w128_r33_axis", 128, 33, 2, "2dim+64", ROPE_AXIS, GRID_B, 7, 11, "qh"),         # 16 chunks: 48 idle lanes
    _rms("w128_r5_token", 128, 5, 1, "dim", ROPE_TOKEN, GRID_A, 0, 0, "q1"),
    _rms("w1280_r17_axis", 1280, 17, 2, "2dim", ROPE_AXIS, GRID_A, 7, 0, "q1"),           # 160 chunks: a partial third chunk, generic MAXC = 3
    _rms("w1280_r4_token", 1280, 4, 2, "2dim+64", ROPE_TOKEN, GRID_B, 0, 2, "qh"),
    _rms("w2048_r16_token", 2048, 16, 2, "2dim", ROPE_TOKEN, GRID_B, 7, 8, "q1"),         # generic MAXC = 10
    _rms("w2048_r5_norope", 2048, 5, 1, "2dim", ROPE_NONE, scales="11"),
    _rms("w8192_r5_axis", 8192, 5, 2, "2dim", ROPE_AXIS, GRID_A, 7, 0, "qh"),             # MAXC = 16
    _rms("w8192_r3_norope", 8192, 3, 1, "dim", ROPE_NONE, scales="q1"),
]
RMS_BY_NAME = {c["name"]: c for c in RMS_CASES}


def rms_ld(case):
    return {"dim": case["dim"], "2dim": 2 * case["dim"], "2dim+64": 2 * case["dim"] + 64}[case["ld"]]


def rms_edge_rows(rows):
    """{edge: row} of the single rows that carry an input edge (none below 5 rows: those cases are the row-walk's ends)."""
    return {"zero": 1, "tiny": 2, "huge": rows - 1} if rows >= 5 else {}


FILL = -1.0078125          # a bf16 value: what every element the launch does not own holds before and must hold after


def rms_inputs(case, seed=None):
    """(x [rows + GUARD_ROWS, ld] fp32 holding bf16 values, weight_q, weight_k): random rows of spread 2 with the edge rows set in, FILL elsewhere."""
    dim, rows, ld = case["dim"], case["rows"], rms_ld(case)
    rs = np.random.RandomState(sum(map(ord, case["name"])) * 7 + 11 if seed is None else seed)
    x = np.full((rows + GUARD_ROWS, ld), FILL, dtype=np.float32)
    span = min(ld, 2 * dim)
    x[:rows, :span] = rbf32((2 * rs.standard_normal((rows, span))).astype(np.float32))
    for edge, r in rms_edge_rows(rows).items():
        x[r, :span] *= {"zero": 0.0, "tiny": 2.0 ** -40, "huge": 2.0 ** 40}[edge]
    wq = rbf32((1 + 0.1 * rs.standard_normal(dim)).astype(np.float32))
    wk = rbf32((1 + 0.1 * rs.standard_normal(dim)).astype(np.float32))
    return x, wq, wk


def rms_tokens(case):
    """Token of every row: row0 + row, or row0 + row % period for stacked samples."""
    r = np.arange(case["rows"])
    return case["row0"] + (r % case["period"] if case["period"] > 0 else r)


@functools.lru_cache(maxsize=None)
def rope_table_f32(grid):
    """(cos, sin) [f h w, 64]: the fp64 table as the kernels hold it, in fp32."""
    t = wdo.rope_table_3d(128, grid)
    return t.real.numpy().astype(np.float32), t.imag.numpy().astype(np.float32)


def rms_reference_operand(x, weight, out_scale, tokens=None, grid=None):
    """fp64 reference of one operand x [rows, dim]: (want, s)."""
    xt = torch.from_numpy(np.asarray(x, dtype=np.float64))
    y = wdo.rms_norm_full(xt, torch.from_numpy(np.asarray(weight, dtype=np.float64)), EPS, _rnd_t).numpy()
    if tokens is None:
        want = rbf64(y * out_scale)
        return want, np.abs(want)
    cos, sin = (t[tokens].astype(np.float64) for t in rope_table_f32(grid))           # [rows, 64]
    rows, dim = y.shape
    yp = y.reshape(rows, dim // 128, 64, 2)
    a, b, c, s = yp[..., 0], yp[..., 1], cos[:, None, :], sin[:, None, :]
    want = rbf64(np.stack([(a * c - b * s) * out_scale, (a * s + b * c) * out_scale], axis=-1)).reshape(rows, dim)
    mag = np.repeat(((np.abs(a) + np.abs(b)) * out_scale)[..., None], 2, axis=-1).reshape(rows, dim)
    return want, mag


def rms_emulate_operand(x, weight, out_scale, tokens=None, grid=None):
    """The kernels' fp32 order on one operand x [rows, dim] -> bf16 values in fp32."""
    x = np.asarray(x, dtype=np.float32)
    rows, dim = x.shape
    ss = _wave_tree(_lane_partials(x * x))
    rs = _rsqrt32(ss / np.float32(dim) + np.float32(EPS))[:, None]
    y = rbf32(rbf32(x * rs) * np.asarray(weight, dtype=np.float32))
    sc = np.float32(out_scale)
    if tokens is None:
        return rbf32(y * sc)
    cos, sin = (t[tokens][:, None, :] for t in rope_table_f32(grid))
    yp = y.reshape(rows, dim // 128, 64, 2)
    a, b = yp[..., 0], yp[..., 1]
    return rbf32(np.stack([(a * cos - b * sin) * sc, (a * sin + b * cos) * sc], axis=-1).astype(np.float32)).reshape(rows, dim)


def _operands(case, x, wq, wk):
    dim, rows = case["dim"], case["rows"]
    sq, sk = SCALES[case["scales"]]
    ops = [(0, wq, sq)] + ([(dim, wk, sk)] if case["nop"] == 2 else [])
    tok = rms_tokens(case) if case["rope"] else None
    return [(c0, x[:rows, c0:c0 + dim], w, sc, tok) for c0, w, sc in ops]


@functools.lru_cache(maxsize=None)
def rms_reference(name):
    """(want, s) over the whole [rows + GUARD_ROWS, ld] buffer: outside the operands want is the input (FILL, or the untouched half) and s = 0."""
    case = RMS_BY_NAME[name]
    x, wq, wk = rms_inputs(case)
    want, s = x.astype(np.float64), np.zeros(x.shape)
    for c0, xo, w, sc, tok in _operands(case, x, wq, wk):
        want[:case["rows"], c0:c0 + case["dim"]], s[:case["rows"], c0:c0 + case["dim"]] = rms_reference_operand(xo, w, sc, tok, case["grid"])
    want.setflags(write=False); s.setflags(write=False)
    return want, s


def rms_emulation(name):
    case = RMS_BY_NAME[name]
    x, wq, wk = rms_inputs(case)
    out = x.copy()
    for c0, xo, w, sc, tok in _operands(case, x, wq, wk):
        out[:case["rows"], c0:c0 + case["dim"]] = rms_emulate_operand(xo, w, sc, tok, case["grid"])
    return out


def rms_owned(case):
    """Boolean [rows + GUARD_ROWS, ld]: the elements the launch writes."""
    m = np.zeros((case["rows"] + GUARD_ROWS, rms_ld(case)), dtype=bool)
    m[:case["rows"], :case["nop"] * case["dim"]] = True
    return m


# ------------------------------------------------------------------------------------------------ LayerNorm cases
LN_MODES = ("plain", "affine", "mod", "affine+mod")


def _ln_cases():
    out = [dict(name=f"w{dim}_r{rows}_{mode}", dim=dim, rows=rows, mode=mode) for dim in MULTI_ROW_DIMS for rows in ROW_COUNTS for mode in ("affine", "mod")]
    out += [dict(name=f"w{dim}_r{rows}_{mode}", dim=dim, rows=rows, mode=mode) for dim in MULTI_ROW_DIMS for rows, mode in ((17, "plain"), (5, "affine+mod"))]
    out += [dict(name=f"w{dim}_r{rows}_{mode}", dim=dim, rows=rows, mode=mode)
            for dim, rows, mode in ((128, 33, "mod"), (128, 5, "affine"), (1280, 17, "mod"), (1280, 5, "affine+mod"), (2048, 16, "affine"), (2048, 5, "plain"),
                                    (8192, 5, "mod"), (8192, 3, "affine"))]
    return out


LN_CASES = _ln_cases()
LN_BY_NAME = {c["name"]: c for c in LN_CASES}
LN_CONSTANT = -2.5          # dim copies of it sum exactly in fp32 in any order, so mean = x and the output is bias / shift to the bit


def ln_edge_rows(rows):
    return {"constant": 1, "zero": 2, "mean8": rows - 1} if rows >= 5 else {}


def ln_inputs(case, seed=None):
    """(x [rows, dim], w, b, shift, scale) as fp32 arrays of bf16 values; w / b and shift / scale are None where the mode has none."""
    dim, rows, mode = case["dim"], case["rows"], case["mode"]
    rs = np.random.RandomState(sum(map(ord, case["name"])) * 5 + 3 if seed is None else seed)
    x = rbf32((3 * rs.standard_normal((rows, dim)) + 0.5).astype(np.float32))
    off = np.rint(4 * rs.standard_normal(dim // 2)) / 16          # spread 0.25 on bf16's grid at 8 (spacing 1/16)
    mean8 = rs.permutation(np.concatenate([8 + off, 8 - off]))
    for edge, r in ln_edge_rows(rows).items():
        x[r] = {"constant": np.full(dim, LN_CONSTANT), "zero": np.zeros(dim), "mean8": mean8}[edge]
    w = rbf32((1 + 0.1 * rs.standard_normal(dim)).astype(np.float32))
    b = rbf32((0.1 * rs.standard_normal(dim)).astype(np.float32))
    sh = rbf32((0.3 * rs.standard_normal(dim)).astype(np.float32))
    sc = rbf32((0.3 * rs.standard_normal(dim)).astype(np.float32))
    return x, (w if "affine" in mode else None), (b if "affine" in mode else None), (sh if "mod" in mode else None), (sc if "mod" in mode else None)


def ln_reference_arrays(x, w, b, sh, sc):
    """fp64 reference of x [rows, dim]."""
    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a, dtype=np.float64))
    xt = t(x)
    if sh is None:
        return rbf64(wdo.layer_norm(xt, EPS, t(w), t(b)).numpy())
    if w is None:
        return wdo.modulated_norm(xt, t(sh), t(sc), EPS, _rnd_t).numpy()
    y = rbf64(wdo.layer_norm(xt, EPS, t(w), t(b)).numpy())          # affine + modulated: the affine result is the bf16 tensor the modulation reads
    return rbf64(rbf64(y * rbf64(1.0 + np.asarray(sc, dtype=np.float64))) + sh)


def ln_emulate_arrays(x, w, b, sh, sc):
    x = np.asarray(x, dtype=np.float32)
    dim = x.shape[1]
    mean = (_wave_tree(_lane_partials(x)) / np.float32(dim))[:, None]
    d = x - mean
    rstd = _rsqrt32(_wave_tree(_lane_partials(d * d)) / np.float32(dim) + np.float32(EPS))[:, None]
    y = d * rstd
    if w is not None:
        y = y * w + b
    y = rbf32(y)
    if sh is not None:
        y = rbf32(rbf32(y * rbf32(np.float32(1) + sc)) + sh)
    return y


@functools.lru_cache(maxsize=None)
def ln_reference(name):
    want = ln_reference_arrays(*ln_inputs(LN_BY_NAME[name]))
    want.setflags(write=False)
    return want


def ln_emulation(name):
    return ln_emulate_arrays(*ln_inputs(LN_BY_NAME[name]))


# ------------------------------------------------------------------------------------------------ the kernels' summation order
def _lane_partials(v):
    """[rows, dim] fp32 -> [rows, 64]: lane l adds the elements of chunks l, l + 64, ... (8 each) one after the other."""
    rows, dim = v.shape
    nchunk = dim // 8
    maxc = -(-nchunk // 64)
    pad = np.zeros((rows, maxc * 64, 8), dtype=np.float32)
    pad[:, :nchunk] = v.reshape(rows, nchunk, 8)
    pad = pad.reshape(rows, maxc, 64, 8)
    acc = np.zeros((rows, 64), dtype=np.float32)
    for c in range(maxc):
        for j in range(8):
            acc = acc + pad[:, c, :, j]
    return acc


def _wave_tree(p):
    """wave_sum: v += shfl_xor(v, o) for o = 32 .. 1; every lane ends with the same sum."""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        p = p + p[:, lanes ^ o]
    return p[:, 0]


def _rsqrt32(v):
    return (1.0 / np.sqrt(v.astype(np.float64))).astype(np.float32)
