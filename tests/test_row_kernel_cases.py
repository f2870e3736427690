"""The case tables, references and bound of the row-kernel GPU tests (tests/row_kernel_cases.py), checked on the host: for every case the
fp32 emulation of the kernels' operation order meets the per-element bound against the fp64 reference with its moved roundings under the
cap in every row (a condition on the cases: where one exceeds it, its inputs change, not the cap); the tables hold every width, row
count, launch argument and input edge the GPU file is about; and the launcher's choice of kernel, restated here, says which cases reach
the four-rows-per-wave kernels."""
import json

import numpy as np
import pytest

import row_kernel_cases as rk


def rms_kernel(case, rms_rows=1):
    """svi_launch_rmsnorm_rope2's choice: ("rows" | "generic", MAXC)."""
    nchunk = case["dim"] // 8
    if nchunk in (64 * 3, 64 * 10) and case["rope"] in (rk.ROPE_NONE, rk.ROPE_TOKEN) and rms_rows:
        return "rows", nchunk // 64
    return "generic", 3 if nchunk <= 64 * 3 else 10 if nchunk <= 64 * 10 else 16


def ln_kernel(case, rms_rows=1):
    """svi_launch_ln_mod's choice: the multi-row kernel for whole chunks per lane and exactly one of affine / modulated."""
    nchunk = case["dim"] // 8
    if nchunk in (64 * 3, 64 * 10) and case["mode"] in ("affine", "mod") and rms_rows:
        return "rows", nchunk // 64
    return "generic", 3 if nchunk <= 64 * 3 else 10 if nchunk <= 64 * 10 else 16


def _line(kind, name, v):
    print(json.dumps({"test": kind, "case": name, **v}))


@pytest.mark.parametrize("name", [c["name"] for c in rk.RMS_CASES])
def test_rms_emulation_meets_the_bound(name):
    want, s = rk.rms_reference(name)
    v = rk.verdict(rk.rms_emulation(name), want, s)
    _line("rms_emulation", name, v)
    assert v["bad"] == 0, v
    assert v["worst_row_share"] < rk.MOVED_CAP, v


@pytest.mark.parametrize("name", [c["name"] for c in rk.LN_CASES])
def test_ln_emulation_meets_the_bound(name):
    v = rk.verdict(rk.ln_emulation(name), rk.ln_reference(name))
    _line("ln_emulation", name, v)
    assert v["bad"] == 0, v
    assert v["worst_row_share"] < rk.MOVED_CAP, v


def test_rounding_helpers():
    v = np.array([1.0, 1.00390625, 1.01171875, -3.0e-12, 2.0 ** 40 * 1.0078125, 0.0, 255.5])
    assert np.array_equal(rk.rbf64(v), rk.rbf32(v.astype(np.float32)).astype(np.float64))
    assert rk.rbf64(1.00390625) == 1.0 and rk.rbf64(1.01171875) == 1.015625          # ties to even, both ways
    assert rk.rbf64(1.0 + 2.0 ** -8 + 2.0 ** -40) == 1.0078125                        # one rounding: fp64 -> fp32 -> bf16 would give 1.0
    assert rk.bf16_ulp(1.0) == 2.0 ** -7 and rk.bf16_ulp(1.99) == 2.0 ** -7 and rk.bf16_ulp(0.0) == 0.0
    assert rk.rbf32(np.float32(rk.FILL)) == np.float32(rk.FILL) and rk.rbf32(np.float32(rk.LN_CONSTANT)) == np.float32(rk.LN_CONSTANT)


def test_the_bound_sorts_equal_moved_and_wrong():
    want = np.array([[1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 1.9921875]])
    got = np.array([[1.0, 1.0078125, 1.015625, 1.0234375, 0.0, 1e-30, 2.0]])
    moved, bad = rk.judge(got, want)
    assert moved.tolist() == [[False, True, True, False, False, False, True]]           # one and two ulps off, also at the top of a binade: only equality meets the bound
    assert bad.tolist() == [[False, False, False, True, False, True, False]]            # three ulps off; anything where zero is due
    # a cancelling pair: the noise and the window are relative to the pair's inputs
    moved, bad = rk.judge(np.array([0.0078125 + 2.0 ** -21, 0.0078125 + 2.0 ** -8, 0.0078125 + 2.0 ** -4]), np.full(3, 0.0078125), np.full(3, 2.0))
    assert moved.tolist() == [False, True, False] and bad.tolist() == [False, False, True]
    assert rk.judge(np.array([np.nan, np.inf]), np.array([1.0, 1.0]))[1].all()


def test_rms_table_holds_every_axis_of_the_launch():
    cs = rk.RMS_CASES
    assert len({c["name"] for c in cs}) == len(cs)
    assert {c["dim"] for c in cs} == {128, 1280, 1536, 2048, 5120, 8192}
    reached = {rms_kernel(c) for c in cs}
    assert reached >= {("rows", 3), ("rows", 10), ("generic", 3), ("generic", 10), ("generic", 16)}
    assert rms_kernel(rk.RMS_BY_NAME["w1280_r17_axis"]) == ("generic", 3) and 1280 // 8 == 2 * 64 + 32          # a partial third chunk
    assert rms_kernel(rk.RMS_BY_NAME["w2048_r16_token"]) == ("generic", 10) and rms_kernel(rk.RMS_BY_NAME["w128_r5_token"]) == ("generic", 3)
    for dim in rk.MULTI_ROW_DIMS:          # every row count on the production kernel with RoPE, and the kernel without RoPE
        prod = [c for c in cs if c["dim"] == dim and c["rope"] == rk.ROPE_TOKEN]
        assert sorted(c["rows"] for c in prod) == list(rk.ROW_COUNTS) and all(rms_kernel(c)[0] == "rows" for c in prod)
        assert any(c["dim"] == dim and c["rope"] == rk.ROPE_NONE and rms_kernel(c)[0] == "rows" for c in cs)
        assert any(c["dim"] == dim and c["rope"] == rk.ROPE_AXIS for c in cs)
        assert {c["ld"] for c in prod} == {"dim", "2dim", "2dim+64"} and {c["scales"] for c in prod} == set(rk.SCALES)
        assert {c["row0"] for c in prod} == {0, 7}
        assert {0} | {c["rows"] // 2 for c in prod if c["period"] and c["period"] * 2 == c["rows"]} | {c["rows"] // 3 for c in prod if c["period"] * 3 == c["rows"]} \
            <= {c["period"] for c in prod}
        assert any(c["period"] * 2 == c["rows"] for c in prod) and any(c["period"] * 3 == c["rows"] for c in prod) and any(c["period"] == 0 for c in prod)
        assert any(c["nop"] == 1 and c["ld"] == "2dim" for c in prod)          # the other half of the row must stay
    assert rk.ROW_COUNTS == (1, 3, 4, 5, 15, 16, 17, 33)
    assert rk.SCALES == {"11": (1.0, 1.0), "q1": (rk.QK_SCALE, 1.0), "qh": (rk.QK_SCALE, 0.5)}
    assert abs(rk.QK_SCALE - 1.4426950408889634 / np.sqrt(128)) < 1e-8
    for c in cs:
        f, h, w = c["grid"]
        assert c["nop"] in (1, 2) and (c["nop"] == 1 or c["ld"] != "dim") and rk.rms_ld(c) % 8 == 0
        if c["rope"]:          # what the launcher requires, and a shard: fewer rows than the grid has tokens
            assert f > 1 and h != w and c["dim"] % 128 == 0
            tok = rk.rms_tokens(c)
            assert tok.min() == c["row0"] and tok.max() < f * h * w and c["rows"] < f * h * w
            assert c["period"] == 0 or (c["rows"] % c["period"] == 0 and c["row0"] + c["period"] <= f * h * w)
            assert c["row0"] in (0, 7) and (c["row0"] == 0 or 0 < c["row0"] % w)          # 7 lies inside a grid row
    assert any(c["rope"] and c["grid"] == rk.GRID_A for c in cs) and any(c["rope"] and c["grid"] == rk.GRID_B for c in cs)


def test_rms_inputs_hold_every_edge_row():
    seen = set()
    for c in rk.RMS_CASES:
        x, wq, wk = rk.rms_inputs(c)
        span = min(rk.rms_ld(c), 2 * c["dim"])
        assert np.array_equal(x, rk.rbf32(x)) and np.array_equal(wq, rk.rbf32(wq)) and np.array_equal(wk, rk.rbf32(wk))
        assert (x[c["rows"]:] == rk.FILL).all() and (x[:, span:] == rk.FILL).all()
        edges = rk.rms_edge_rows(c["rows"])
        want, s = rk.rms_reference(c["name"])
        own = rk.rms_owned(c)
        assert np.array_equal(want[~own], x[~own].astype(np.float64)) and (s[~own] == 0).all()
        for edge, r in edges.items():
            row = np.abs(x[r, :span])
            if edge == "zero":
                assert (row == 0).all() and (want[r][own[r]] == 0).all()
            elif edge == "tiny":          # mean x^2 ~ 2^-78 against eps = 1e-6: rs = eps^-1/2, and a dropped eps would give values of order 1
                assert 0 < row.max() < 2.0 ** -36 and float(np.mean(row.astype(np.float64) ** 2)) < 1e-6 * rk.EPS
                assert 0 < np.abs(want[r][own[r]]).max() < 2.0 ** -25
            else:
                assert row.max() > 2.0 ** 38 and np.isfinite(want[r]).all() and 0.01 < np.abs(want[r][own[r]]).max() < 10
            seen.add(edge)
        assert len(set(edges.values())) == len(edges)
    assert seen == {"zero", "tiny", "huge"}
    for dim in rk.MULTI_ROW_DIMS:          # on the production kernel too
        assert any(c["dim"] == dim and c["rope"] == rk.ROPE_TOKEN and rk.rms_edge_rows(c["rows"]) for c in rk.RMS_CASES)


def test_ln_table_and_inputs_hold_every_form_and_edge():
    cs = rk.LN_CASES
    assert len({c["name"] for c in cs}) == len(cs)
    assert {c["dim"] for c in cs} == {128, 1280, 1536, 2048, 5120, 8192} and {c["mode"] for c in cs} == set(rk.LN_MODES)
    for dim in rk.MULTI_ROW_DIMS:
        for mode in ("affine", "mod"):
            walk = [c for c in cs if c["dim"] == dim and c["mode"] == mode]
            assert sorted(c["rows"] for c in walk) == list(rk.ROW_COUNTS) and all(ln_kernel(c) == ("rows", dim // 512) for c in walk)
        for mode in ("plain", "affine+mod"):          # these stay on the generic kernel at the DiT's widths
            assert any(c["dim"] == dim and c["mode"] == mode and ln_kernel(c)[0] == "generic" for c in cs)
    assert {ln_kernel(c) for c in cs} >= {("rows", 3), ("rows", 10), ("generic", 3), ("generic", 10), ("generic", 16)}
    seen = set()
    for c in cs:
        x, w, b, sh, sc = rk.ln_inputs(c)
        assert np.array_equal(x, rk.rbf32(x)) and (w is None) == (b is None) == ("affine" not in c["mode"]) and (sh is None) == (sc is None) == ("mod" not in c["mode"])
        want = rk.ln_reference(c["name"])
        for edge, r in rk.ln_edge_rows(c["rows"]).items():
            if edge in ("constant", "zero"):          # the output is the last vector added, to the bit
                assert (x[r] == (rk.LN_CONSTANT if edge == "constant" else 0)).all()
                due = (sh if sh is not None else b if b is not None else np.zeros(c["dim"])).astype(np.float64)
                if c["mode"] == "affine+mod":          # the affine form's result, bias, is what the modulation reads
                    due = rk.rbf64(rk.rbf64(b * rk.rbf64(1.0 + sc.astype(np.float64))) + sh)
                assert np.array_equal(want[r], due), (c["name"], edge)
            else:
                assert abs(float(x[r].astype(np.float64).mean()) - 8) == 0 and 0.2 < float(x[r].astype(np.float64).std()) < 0.35
            seen.add(edge)
    assert seen == {"constant", "zero", "mean8"}


def test_a_wrong_kernel_would_miss_the_bound():
    """The bound is not slack: the neighbouring token's table row, a second rounding around the output scale, a statistic off by 2^-9 and a
    dropped eps each leave the reference by more than the bound and the cap admit."""
    c = rk.RMS_BY_NAME["w1536_r17"]
    x, wq, wk = rk.rms_inputs(c)
    xo, tok = x[:c["rows"], :c["dim"]], rk.rms_tokens(c)
    want, s = rk.rms_reference_operand(xo, wq, rk.QK_SCALE, tok, c["grid"])
    for wrong in (rk.rms_emulate_operand(xo, wq, rk.QK_SCALE, tok + 1, c["grid"]),                          # the next token's pairs
                  rk.rbf32(rk.rms_emulate_operand(xo, wq, 1.0, tok, c["grid"]) * np.float32(rk.QK_SCALE)),      # a second rounding around the scale
                  rk.rms_emulate_operand(xo * np.float32(1 + 2.0 ** -9), wq, rk.QK_SCALE, tok, c["grid"])):
        v = rk.verdict(wrong, want, s)
        assert v["bad"] > 0 or v["worst_row_share"] > rk.MOVED_CAP, v
    tiny = rk.rms_edge_rows(c["rows"])["tiny"]
    no_eps = xo[tiny].astype(np.float64) / np.sqrt(np.mean(xo[tiny].astype(np.float64) ** 2))
    assert rk.judge(rk.rbf64(no_eps), want[tiny], s[tiny])[1].mean() > 0.9
