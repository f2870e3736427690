"""-m gpu: the row kernels of csrc/svi_elementwise.hip in the forms the DiT block launches them.

RMSNorm + RoPE goes through svi_rmsnorm_rope_qk, the seam of the block's own q | k launch (two operands side by side in a row, the attention
scale folded into q, a shard's first token, the stacked CFG pair's period, the per-token table): at dim 1536 / 5120 with rope = 2 that is
rmsnorm_rope_rows_kernel<3 | 10, 4, true>, the kernel under every self-attention.  LayerNorm goes through svi_layernorm_modulate.

Three kinds of check (cases, references and the bound: tests/row_kernel_cases.py, held on the host by tests/test_row_kernel_cases.py):
  * every element against the fp64 reference under the per-element bound, moved roundings at most 2e-3 of the elements of every row, the
    edge rows (zero, 2^-40, 2^40; constant, zero, mean 8) among random ones, and every byte the launch does not own unchanged;
  * torch.equal between forms that must give the same bits: four rows per wave against one, the per-token table against the axis tables,
    two operands against one at a time, a shard against the slice of the whole, a stack against its samples;
  * refusals: a non-zero status and x unchanged.
"""
import numpy as np
import pytest
import torch

import row_kernel_cases as rk
from gpu_util import dev, host, report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import svi_hip
    assert svi_hip._lib.lib().svi_device_count() >= 1
    return svi_hip


class one_row_per_wave:
    """SVI_RMS_ROWS=0 for the duration: the generic kernels also at the DiT's widths."""
    def __init__(self, hip):
        self.L = hip._lib

    def __enter__(self):
        self.L.set_switch("SVI_RMS_ROWS", 0)

    def __exit__(self, *exc):
        self.L.set_switch("SVI_RMS_ROWS", None)


def qk(hip, x, rows, dim, wq, wk=None, scales=(1.0, 1.0), rope=0, grid=(0, 0, 0), row0=0, period=0, expect_ok=True):
    """One svi_rmsnorm_rope_qk launch on a device copy of x (numpy [>= rows, ld]); returns (status, result on the host as fp32)."""
    xd = dev(x)
    st = hip.ops.rmsnorm_rope_qk_(xd, rows, dim, dev(wq), None if wk is None else dev(wk), rk.EPS, scales[0], scales[1], rope, grid, row0, period)
    torch.cuda.synchronize()
    if expect_ok:
        assert st == 0, (st, hip._lib.last_error())
    return st, host(xd).numpy()


def run_case(hip, c, rope=None):
    x, wq, wk = rk.rms_inputs(c)
    return qk(hip, x, c["rows"], c["dim"], wq, wk if c["nop"] == 2 else None, rk.SCALES[c["scales"]], c["rope"] if rope is None else rope,
              c["grid"], c["row0"], c["period"])[1]


def ln(hip, inputs):
    x, w, b, sh, sc = inputs
    d = lambda a: None if a is None else dev(a)
    out = hip.layernorm_modulate(dev(x), rk.EPS, weight=d(w), bias=d(b), shift=d(sh), scale=d(sc))
    torch.cuda.synchronize()
    return host(out).numpy()


# ------------------------------------------------------------------------------------------------ against the fp64 reference
@pytest.mark.parametrize("name", [c["name"] for c in rk.RMS_CASES])
def test_rmsnorm_rope_qk_against_fp64(hip, name):
    c = rk.RMS_BY_NAME[name]
    x = rk.rms_inputs(c)[0]
    got = run_case(hip, c)
    want, s = rk.rms_reference(name)
    own = rk.rms_owned(c)
    v = rk.verdict(got[:c["rows"], :c["nop"] * c["dim"]], want[:c["rows"], :c["nop"] * c["dim"]], s[:c["rows"], :c["nop"] * c["dim"]])
    report("row_rmsnorm_rope_qk", case=name, **v)
    print(name, v)
    assert v["bad"] == 0, v
    assert v["worst_row_share"] <= rk.MOVED_CAP, v
    # guard columns, rows past `rows`, and with one operand in a two-operand row the other half: the bits they had
    assert np.array_equal(got[~own], x[~own]), f"{name}: the launch wrote {int((got[~own] != x[~own]).sum())} elements it does not own"
    edges = rk.rms_edge_rows(c["rows"])
    if edges:
        assert (got[edges["zero"]][own[edges["zero"]]] == 0).all()
        assert np.isfinite(got).all()


@pytest.mark.parametrize("name", [c["name"] for c in rk.LN_CASES])
def test_layernorm_modulate_against_fp64(hip, name):
    c = rk.LN_BY_NAME[name]
    inputs = rk.ln_inputs(c)
    got = ln(hip, inputs)
    want = rk.ln_reference(name)
    v = rk.verdict(got, want)
    report("row_layernorm_modulate", case=name, **v)
    print(name, v)
    assert v["bad"] == 0, v
    assert v["worst_row_share"] <= rk.MOVED_CAP, v
    edges = rk.ln_edge_rows(c["rows"])
    for edge in ("constant", "zero"):          # (x - mean) is exactly zero: the output is the reference's to the bit (bias, or shift)
        if edge in edges:
            assert np.array_equal(got[edges[edge]].astype(np.float64), want[edges[edge]]), (name, edge)


# ------------------------------------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize("dim", rk.MULTI_ROW_DIMS)
def test_four_rows_per_wave_rmsnorm_is_bitwise_one_row_per_wave(hip, dim):
    """SVI_RMS_ROWS=0 against the default at the DiT's widths: every row count, with the per-token table and without RoPE, one and two operands."""
    grid, n = rk.GRID_B, 0
    for rows in rk.ROW_COUNTS:
        for rope in (rk.ROPE_NONE, rk.ROPE_TOKEN):
            for nop in (1, 2):
                c = dict(name=f"sw{dim}_{rows}_{rope}_{nop}", dim=dim, rows=rows, nop=nop, ld="2dim+64", rope=rope, grid=grid, row0=7, period=0, scales="qh")
                x, wq, wk = rk.rms_inputs(c)
                args = (x, rows, dim, wq, wk if nop == 2 else None, rk.SCALES["qh"], rope, grid, 7, 0)
                multi = qk(hip, *args)[1]
                with one_row_per_wave(hip):
                    single = qk(hip, *args)[1]
                assert np.array_equal(multi, single), (dim, rows, rope, nop, int((multi != single).sum()))
                assert not np.array_equal(multi, x)
                n += 1
    assert n == 32


@pytest.mark.parametrize("name", ["w1536_r16", "w1536_r33", "w5120_r15", "w5120_r17", "w128_r33_axis", "w1280_r4_token", "w2048_r16_token", "w8192_r5_axis"])
def test_per_token_table_is_bitwise_the_axis_tables(hip, name):
    c = rk.RMS_BY_NAME[name]
    tok, axis = run_case(hip, c, rope=rk.ROPE_TOKEN), run_case(hip, c, rope=rk.ROPE_AXIS)
    assert np.array_equal(tok, axis), int((tok != axis).sum())
    assert not np.array_equal(tok, run_case(hip, c, rope=rk.ROPE_NONE))


@pytest.mark.parametrize("name", ["w1536_r15", "w1536_r17_norope", "w5120_r33", "w5120_r17_axis", "w1280_r17_axis", "w8192_r5_axis"])
def test_two_operands_are_bitwise_two_launches(hip, name):
    """q | k in one launch against each column half on its own as a one-operand tensor of ld = dim, with its own gain and scale."""
    c = rk.RMS_BY_NAME[name]
    assert c["nop"] == 2
    x, wq, wk = rk.rms_inputs(c)
    rows, dim = c["rows"], c["dim"]
    both = run_case(hip, c)
    for c0, w, sc in ((0, wq, rk.SCALES[c["scales"]][0]), (dim, wk, rk.SCALES[c["scales"]][1])):
        alone = qk(hip, np.ascontiguousarray(x[:rows, c0:c0 + dim]), rows, dim, w, None, (sc, 7.0), c["rope"], c["grid"], c["row0"], c["period"])[1]
        assert np.array_equal(both[:rows, c0:c0 + dim], alone), (name, c0)


@pytest.mark.parametrize("dim,rope", [(1536, rk.ROPE_TOKEN), (5120, rk.ROPE_TOKEN), (1536, rk.ROPE_AXIS), (2048, rk.ROPE_TOKEN)])
def test_a_shard_is_bitwise_the_slice_of_the_whole(hip, dim, rope):
    f, h, w = grid = rk.GRID_A
    L = f * h * w
    c = dict(name=f"whole{dim}", dim=dim, rows=L, nop=2, ld="2dim", rope=rope, grid=grid, row0=0, period=0, scales="q1")
    x, wq, wk = rk.rms_inputs(c)
    whole = qk(hip, x, L, dim, wq, wk, rk.SCALES["q1"], rope, grid, 0, 0)[1]
    for n in (1, 5, 17, L - 7):
        shard = qk(hip, np.ascontiguousarray(x[7:7 + n]), n, dim, wq, wk, rk.SCALES["q1"], rope, grid, 7, 0)[1]
        assert np.array_equal(shard, whole[7:7 + n]), (dim, rope, n)
    assert not np.array_equal(whole[7:8], whole[8:9])


@pytest.mark.parametrize("dim,rope,nb", [(1536, rk.ROPE_TOKEN, 2), (1536, rk.ROPE_TOKEN, 3), (5120, rk.ROPE_TOKEN, 2), (5120, rk.ROPE_TOKEN, 3), (1280, rk.ROPE_AXIS, 2)])
def test_a_stack_with_period_is_bitwise_its_samples(hip, dim, rope, nb):
    grid, per = rk.GRID_B, 11          # 11 rows per sample: a sample's first row falls on every position of a wave's walk
    c = dict(name=f"stack{dim}_{nb}", dim=dim, rows=nb * per, nop=2, ld="2dim", rope=rope, grid=grid, row0=7, period=per, scales="qh")
    x, wq, wk = rk.rms_inputs(c)
    stack = qk(hip, x, nb * per, dim, wq, wk, rk.SCALES["qh"], rope, grid, 7, per)[1]
    for i in range(nb):
        alone = qk(hip, np.ascontiguousarray(x[i * per:(i + 1) * per]), per, dim, wq, wk, rk.SCALES["qh"], rope, grid, 7, 0)[1]
        assert np.array_equal(stack[i * per:(i + 1) * per], alone), (dim, nb, i)


@pytest.mark.parametrize("dim", rk.MULTI_ROW_DIMS)
def test_four_rows_per_wave_layernorm_is_bitwise_one_row_per_wave(hip, dim):
    """The affine and the modulated form take ln_mod_rows_kernel at these widths; the plain and the affine + modulated form stay on the generic kernel."""
    for rows in rk.ROW_COUNTS:
        for mode in rk.LN_MODES:
            inputs = rk.ln_inputs(dict(name=f"sw{dim}_{rows}_{mode}", dim=dim, rows=rows, mode=mode))
            multi = ln(hip, inputs)
            with one_row_per_wave(hip):
                single = ln(hip, inputs)
            assert np.array_equal(multi, single), (dim, rows, mode, int((multi != single).sum()))


# ------------------------------------------------------------------------------------------------ refusals
def test_the_launcher_refuses_what_it_cannot_run(hip):
    """Each of these returns a non-zero status and leaves x as it was."""
    grid = rk.GRID_A          # 30 tokens
    dim, rows = 256, 12
    x = rk.rbf32((np.random.RandomState(5).standard_normal((rows, 2 * dim))).astype(np.float32))
    w = np.ones(dim, dtype=np.float32)
    big = 8192 + 128
    refused = {
        "grid does not cover [row0, row0 + rows)": dict(rows=rows, dim=dim, wk=w, rope=rk.ROPE_TOKEN, grid=grid, row0=19),
        "grid does not cover rows (axis tables)": dict(rows=rows, dim=dim, wk=w, rope=rk.ROPE_AXIS, grid=(1, 2, 5)),
        "period does not divide rows": dict(rows=rows, dim=dim, wk=w, rope=rk.ROPE_TOKEN, grid=grid, period=5),
        "row0 + period past the grid": dict(rows=rows, dim=dim, wk=w, rope=rk.ROPE_TOKEN, grid=grid, row0=25, period=6),
        "negative row0": dict(rows=rows, dim=dim, wk=w, rope=rk.ROPE_AXIS, grid=grid, row0=-1),
        "weight_k with ld < 2 dim": dict(rows=rows, dim=320, wk=np.ones(320, dtype=np.float32), rope=rk.ROPE_NONE),
        "RoPE with dim % 128 != 0": dict(rows=rows, dim=192, rope=rk.ROPE_AXIS, grid=grid),
        "RoPE with dim % 128 != 0 (per-token table)": dict(rows=rows, dim=320, rope=rk.ROPE_TOKEN, grid=grid),
    }
    for what, a in refused.items():
        wq = np.ones(a["dim"], dtype=np.float32)
        st, after = qk(hip, x, a["rows"], a["dim"], wq, a.get("wk"), (1.0, 1.0), a["rope"], a.get("grid", (0, 0, 0)), a.get("row0", 0), a.get("period", 0), expect_ok=False)
        assert st != 0, what
        assert hip._lib.last_error(), what
        assert np.array_equal(after, x), what
    xb = rk.rbf32(np.random.RandomState(6).standard_normal((2, big)).astype(np.float32))
    st, after = qk(hip, xb, 2, big, np.ones(big, dtype=np.float32), None, (1.0, 1.0), rk.ROPE_NONE, expect_ok=False)
    assert st != 0 and "8192" in hip._lib.last_error() and np.array_equal(after, xb)
    # and the same tensor is accepted where the arguments are in range: the refusals above are not the seam refusing everything
    st, after = qk(hip, x, rows, dim, w, w, (1.0, 1.0), rk.ROPE_TOKEN, grid, 18, 0)
    assert st == 0 and not np.array_equal(after, x)
