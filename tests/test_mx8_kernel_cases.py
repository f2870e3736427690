"""The case table, operands, reference, emulation and arenas of the MX-fp8 kernel GPU tests (tests/mx8_kernel_cases.py), checked on the host: every
case builds with the stated poison and its sums fit the grid; the fp32 emulation equals the fp64 reference to the bit wherever the epilogue is exact
and meets the bound, with its moved roundings under the cap, under the three activations and the fp32 gate; the figures the module's docstring states
are the ones measured; every planted fault is caught, and in the way that fault should be; the table expectations are the oracle's dequantisation;
the quantiser's inputs hold the ties, saturations and blocks they claim; and the table holds every edge the GPU file is about."""
import json

import numpy as np
import pytest
import torch

import gemm_kernel_cases as gk
import mx8_kernel_cases as mk
from oracle import mx8_oracle as mx
from row_kernel_cases import FILL, GUARD_ROWS, MOVED_CAP, rbf64

ALL = list(mk.BY_NAME)
GEMM = [c["name"] for c in mk.CASES + mk.WSC_CASES + [mk.SEAM]]
_seen = {}


def _emulated(name):
    """(reference, emulation, verdict, noise) of a case, once."""
    if name not in _seen:
        ref, emu = mk.reference(name), mk.emulate(name)
        _seen[name] = (ref, emu, mk.verdict(emu["out"], ref["want"], ref["s"]), mk.noise_units(ref, emu))
    return _seen[name]


# ------------------------------------------------------------------------------------------------ arenas
@pytest.mark.parametrize("name", ALL)
def test_case_builds_with_poisoned_arenas(name):
    case, d, ops = mk.BY_NAME[name], mk.dims(mk.BY_NAME[name]), mk.operands(name)
    M, N, K, wsc = case["M"], case["N"], case["K"], case["wsc"]
    S = N if wsc else M
    ar = mk.arenas(case)
    # what the launchers require
    assert K % 128 == 0 and d["lda"] % 16 == 0 and d["ldw"] % 16 == 0 and d["ldc"] % 8 == 0 and d["ldres"] % 8 == 0 and d["lda"] >= K and d["ldw"] >= K
    assert d["sc_rows"] % 256 == 0 and d["sc_rows"] in (mk.ceil256(S), mk.ceil256(S) + 256) and ar["SC"][1] % 4 == 0
    assert ar["A8"][1] % 16 == 0 and ar["W8"][1] % 16 == 0 and ar["C"][1] % 8 == 0 and (ar["A8"][1] % 32 == 16) == (name == "s_a_16_not_32")
    # A8 / W8: the block where the offset says, 0x7F in the guard, the pad columns and the rows after
    for key, rows, ld, blk in (("A8", M, d["lda"], ops["a8"]), ("W8", N, d["ldw"], ops["w8"])):
        flat, off = ar[key]
        grid = flat[off:].reshape(rows + GUARD_ROWS, ld)
        assert flat.dtype == np.uint8 and np.array_equal(grid[:rows, :K], blk) and (flat[:off] == mk.NAN8).all() and (grid[rows:] == mk.NAN8).all() and (grid[:, K:] == mk.NAN8).all()
        assert (blk & 0x7F != 0x7F).all()          # no NaN byte inside an operand
    # the scale table: the oracle's layout on the live rows, 0xFF in every row past them and in a slab before and after
    sc, off = ar["SC"]
    tab = sc[off:off + (K // 128) * d["sc_rows"]].reshape(K // 128, d["sc_rows"])
    assert sc.dtype == np.uint32 and off == d["sc_rows"] and len(sc) == (K // 128 + 2) * d["sc_rows"]
    assert np.array_equal(tab[:, :S].astype(np.int64), mx.scale_table(torch.from_numpy(ops["codes"].copy()), d["sc_rows"]).numpy()[:, :S])
    assert (tab[:, S:] == 0xFFFFFFFF).all() and (sc[:off] == 0xFFFFFFFF).all() and (sc[-d["sc_rows"]:] == 0xFFFFFFFF).all()
    assert ((ops["codes"] > 0) & (ops["codes"] < 255)).all()          # codes 0 and 0xFF are no live operands
    # C: FILL outside the owned block (the residual inside it when in place); bias / gate / residual in NaN
    c_flat, c_off = ar["C"]
    own = mk.owned(case)
    assert own.shape == c_flat.shape and own.sum() == M * N and (c_flat[~own] == FILL).all() and own[c_off] and not own[c_off - 1]
    assert mk.c_view(case, c_flat).shape == (M, N) and mk.c_view(case, own).all() and d["ldc"] >= d["c_off"] + N
    if case["res"] == "inplace":
        assert np.array_equal(mk.c_view(case, c_flat), ops["res"])
    if "res" in ar:
        assert np.isfinite(ar["res"][0]).sum() == M * N and ar["res"][1] % 8 == 0 and d["ldres"] != d["ldc"]
    for key in ("bias", "gate"):
        if key in ar:
            flat, off = ar[key]
            assert np.array_equal(flat[off:off + len(ops[key])], ops[key]) and np.isfinite(flat).sum() == len(ops[key]) and (off % 8 == 1) == case["misalign"]
    # the dequantised operands are what the oracle makes of the same bytes and codes
    sc8, codes = (ops["w8"], ops["codes"]) if wsc else (ops["a8"], ops["codes"])
    deq = mx.mx8_dequantize(torch.from_numpy(sc8.copy()).view(torch.float8_e4m3fn), torch.from_numpy(codes.copy())).double().numpy()
    assert np.array_equal(deq, ops["w"] if wsc else ops["a"]) and np.array_equal(mk.DECODE[ops["a8"] if wsc else ops["w8"]], ops["a"] if wsc else ops["w"])
    for v in (ops["bias"], ops["res"]) + (() if case["gate_f32"] else (ops["gate"],)):
        if v is not None:
            assert np.array_equal(rbf64(v), v)          # bf16 values
    if case["special"] is None:          # the grid: multiples of 1/2 up to 3, codes 127 - 3 .. 127 + 3 moved by the edge rows' shift
        body = mk.DECODE[ops["a8"]], mk.DECODE[ops["w8"]]
        assert all(np.array_equal(np.rint(2 * b), 2 * b) and np.abs(b).max() <= 3 for b in body)
        e = ops["codes"].astype(np.int64) - 127 - ops["shift"][:, None]
        assert e.min() >= -3 and e.max() <= 3 and (S < 5 or (np.diff(e, axis=1) != 0).mean() > 0.8 and (np.diff(e, axis=0) != 0).mean() > 0.8)
        assert mk.exactness(name) < 22.0


def test_edge_rows_are_in_the_operands():
    ops = mk.operands("m300")          # no bias: A carries all three
    assert ops["shift"][[1, 2, 299]].tolist() == [0, -40, 40] and (ops["a"][1] == 0).all() and {0x00, 0x80} == set(ops["a8"][1].tolist())
    assert 0 < np.abs(ops["a"][2]).max() <= 2.0 ** -35 and np.abs(ops["a"][299]).max() >= 2.0 ** 37 and (ops["w"][1] == 0).all()
    assert mk.operands("m257")["shift"].max() == 0 and mk.operands("m257")["shift"].min() == -40          # bias along N: no 2^40 row in A
    w = mk.operands("w_n520_bias_n")          # W scaled, bias along N: W carries it, its own bias entry 0
    assert w["shift"][519] == 40 and w["bias"][519] == 0 and mk.operands("w_m300")["shift"].max() == 0
    ref = mk.reference("k8960_ffn2")
    assert (ref["want"][gk.CANCEL_ROW, 0::2] == 0).all() and np.isfinite(ref["want"]).all()


# ------------------------------------------------------------------------------------------------ reference against emulation
@pytest.mark.parametrize("name", GEMM)
def test_emulation_meets_the_bound(name):
    case = mk.BY_NAME[name]
    ref, emu, v, noise = _emulated(name)
    print(json.dumps({"test": "mx8_emulation", "case": name, "noise_acc": noise[0], "noise_last": noise[1], "bits": mk.exactness(name), **v}))
    assert v["bad"] == 0 and v["worst_row_share"] <= MOVED_CAP, v
    assert np.isfinite(ref["want"]).all() and np.array_equal(rbf64(ref["want"]), ref["want"])
    own = mk.owned(case)
    assert np.array_equal(emu["c"][~own], mk.arenas(case)["C"][0][~own])
    # (a bias added to the 2^-40 row: fp32 drops the row's sum, 2^-40 times some hundreds, beside a bias of 2^-3 or more: under 2^-24 S0 / 4, below every rounding)
    assert noise[0] <= (0.25 if case["bias"] is not None else 0.0) and max(noise) <= mk.C_NOISE / 2, noise
    if mk.exact_epilogue(case):
        # (a residual added to the 2^-40 row's result loses in fp32 what fp64 keeps, far below the rounding: the same bits come out)
        assert v["moved"] == 0 and noise[1] <= (0.05 if case["res"] else 0.0) and np.array_equal(emu["out"].astype(np.float64), ref["want"]), v          # the reference's bits


def test_noise_and_moved_share_as_documented():
    rows = {n: _emulated(n) for n in GEMM}
    worst_last = max(r[3][1] for r in rows.values())
    worst_share = max(r[2]["worst_row_share"] for r in rows.values())
    inexact = {n for n, r in rows.items() if r[3][1] > 0.05 or r[2]["moved"]}
    print(worst_last, worst_share, sorted(inexact))
    assert inexact <= {"wide_gelu_tanh", "wide_gelu_erf", "wide_silu", "wide_gate_f32", "wide_gelu_tanh_nobias"}
    assert 1.0 < worst_last <= 1.41 + 1e-2 and worst_share <= 6.5e-4 + 1e-5 and "1.41 (gelu_tanh" in mk.__doc__ and "6.5e-4" in mk.__doc__
    bits = {k: max(mk.exactness(n) for n in GEMM if mk.BY_NAME[n]["K"] == k) for k in (128, 256, 1536, 8960)}
    print(bits)
    assert all(abs(bits[k] - want) < 0.1 for k, want in ((128, 14.7), (256, 15.3), (1536, 16.9), (8960, 19.0))), bits
    assert "14.7 bits at K = 128, 15.3 at 256, 16.9 at 1536, 19.0 at K = 8960" in mk.__doc__
    assert f"{len(mk.CASES)} in CASES + {len(mk.WSC_CASES)} in WSC_CASES + {len(mk.TABLE_CASES)} TABLE_CASES" in mk.__doc__


# ------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("name", [c["name"] for c in mk.TABLE_CASES])
def test_table_expectations_are_the_oracles_dequantisation(name):
    case, ops, ref = mk.BY_NAME[name], mk.operands(name), mk.reference(name)
    scaled8, unit8 = (ops["w8"], ops["a8"]) if case["wsc"] else (ops["a8"], ops["w8"])
    table, eye = (scaled8, unit8) if case["special"] == "table_scaled" else (unit8, scaled8)
    assert set(table.ravel().tolist()) == set(mk.FINITE) and (np.diag(eye) == 0x38).all() and np.count_nonzero(eye) == 256 and mk.DECODE[0x38] == 1.0
    if case["special"] == "table_scaled":
        want = mx.mx8_dequantize(torch.from_numpy(table.copy()).view(torch.float8_e4m3fn), torch.from_numpy(ops["codes"].copy())).double().numpy()
        r, b = np.arange(256)[:, None], np.arange(8)[None, :]
        assert np.array_equal(ops["codes"], 127 + ((5 * r + 11 * b) % 121 - 60)) and ops["codes"].min() == 67 and ops["codes"].max() == 187
        assert (np.diff(ops["codes"].astype(int), axis=1) != 0).all() and (np.diff(ops["codes"].astype(int), axis=0) != 0).all()
    else:
        want = torch.from_numpy(table.copy()).view(torch.float8_e4m3fn).to(torch.bfloat16).double().numpy()
        assert (ops["codes"] == 127).all()
    # the table lies in A (C = it) or in W (C = its transpose): svi_gemm_mx8 scales A, svi_gemm_mx8_wscaled W
    table_in_a = (case["special"] == "table_scaled") != case["wsc"]
    want = want if table_in_a else want.T
    assert np.array_equal(ref["want"], want) and np.array_equal(rbf64(want), want)
    assert (np.abs(want[want != 0]) >= 2.0 ** -100).all()          # normal bf16 numbers throughout
    emu = mk.emulate(name)
    assert np.array_equal(emu["out"].astype(np.float64), want)


# ------------------------------------------------------------------------------------------------ planted faults
def _fails(name, fault):
    """(verdict of the mutated emulation, whether C's unowned part changed)."""
    case, ref = mk.BY_NAME[name], mk.reference(name)
    emu = mk.emulate(name, mutate=fault)
    own = mk.owned(case)
    return mk.verdict(emu["out"], ref["want"], ref["s"]), not np.array_equal(emu["c"][~own], mk.arenas(case)["C"][0][~own], equal_nan=True)


SCALE_TABLES = ("table_scaled", "w_table_scaled")


@pytest.mark.parametrize("fault,names", [("scale_bytes_reversed", SCALE_TABLES + ("m300", "w_k128")), ("scale_blocks_swapped", SCALE_TABLES + ("k128", "w_vt")),
                                         ("scale_row_plus_one", SCALE_TABLES + ("m257", "w_n257"))])
def test_a_scale_from_the_wrong_place_fails(fault, names):
    for name in names:
        v, mask = _fails(name, fault)
        wrong = v["bad"] + v["moved"]
        assert v["bad"] > 0 and not mask, (fault, name, v)
        if name in SCALE_TABLES and fault != "scale_row_plus_one":          # every block differs from the one it is taken for: every non-zero element is off
            assert wrong == np.count_nonzero(mk.reference(name)["want"]), (fault, name, v)
    assert all(_fails(n, None)[0]["bad"] == 0 for n in names)


def test_a_dropped_k_tile_fails():
    for name in ("k128", "k384", "k8960_ffn2", "table_unit", "w_table_scaled", "w_k1536"):
        v, mask = _fails(name, "drop_last_k_tile")
        assert v["bad"] > 0 and not mask, (name, v)
    assert (mk.emulate("table_unit", "drop_last_k_tile")["out"][128:] == 0).all()          # K = [128, 256) is rows 128 .. of the identity's product


def test_a_duplicated_last_row_fails_in_that_row_alone():
    for name in ("m257", "m513", "w_m257", "tn16_m1300"):
        case, ref = mk.BY_NAME[name], mk.reference(name)
        _, bad, _ = mk.judge(mk.emulate(name, "dup_last_row")["out"], ref["want"], ref["s"])
        assert bad[case["M"] - 2].sum() > case["N"] // 2 and not np.delete(bad, case["M"] - 2, axis=0).any(), name


def test_a_pad_column_of_a_read_as_data_fails():
    for name in ("m300", "s_a_16_not_32", "w_m257"):          # lda > K: the pad holds NaN, every output row has one
        v, _ = _fails(name, "read_a_pad")
        assert v["bad"] == mk.BY_NAME[name]["M"] * mk.BY_NAME[name]["N"], (name, v)
    v, _ = _fails("s_ldak_ldc8", "read_a_pad")          # lda == K: the next row's first byte, the guard after the last row
    assert v["bad"] >= mk.BY_NAME["s_ldak_ldc8"]["N"], v


def test_an_element_written_into_cs_pad_fails_the_mask_alone():
    for name in ("m257", "n9", "wide_bias", "s_half_inplace", "w_vt"):
        v, mask = _fails(name, "write_c_pad")
        assert mask and v["bad"] == 0, (name, v)
        assert not _fails(name, None)[1]


def test_a_nan_byte_reaches_its_row_or_column_alone():
    for name in mk.NAN_CASES:
        case, ops = mk.BY_NAME[name], dict(mk.operands(name))
        for key, byte, (r, k) in (("a8", 0x7F, mk.NAN_AT), ("w8", 0xFF, mk.NAN_AT_W)):
            q = ops[key].copy()
            q[r, k] = byte
            codes = ops["codes"]
            a8, w8 = (q, ops["w8"]) if key == "a8" else (ops["a8"], q)
            deq = dict(ops, a=mk.dequantise(a8, None if case["wsc"] else codes), w=mk.dequantise(w8, codes if case["wsc"] else None))
            want = mk.reference_of(case, deq)["want"]
            nan = np.isnan(want)
            assert (nan[r].all() and nan.sum() == case["N"]) if key == "a8" else (nan[:, r].all() and nan.sum() == case["M"]), (name, key)
            assert np.array_equal(want[~nan], mk.reference(name)["want"][~nan])


# ------------------------------------------------------------------------------------------------ the quantiser's inputs
@pytest.mark.parametrize("rows,K", mk.QUANT_SHAPES)
def test_quantiser_inputs_hold_what_they_claim(rows, K):
    x = mk.quant_input(rows, K)
    xt = torch.from_numpy(x).float()
    assert torch.equal(xt.to(torch.bfloat16).float(), xt)
    q, e = mx.mx8_quantize(xt)
    v = x[0, :32] * 2.0 ** (127 - int(e[0, 0]))          # the tie block in units of its scale (2^0)
    codes = np.unique(np.abs(mk.DECODE[np.array(mk.FINITE)]))
    mid = (codes[:-1] + codes[1:]) / 2
    ties = [float(t) for t in v if abs(t) in mid]
    got = mk.DECODE[q.view(torch.uint8).numpy()[0, :32]]
    up = [t for t, g in zip(v, got) if abs(t) in mid and abs(g) > abs(t)]
    down = [t for t, g in zip(v, got) if abs(t) in mid and abs(g) < abs(t)]
    assert int(e[0, 0]) == 127 and len(ties) >= 8 and len(up) >= 3 and len(down) >= 3, (ties, up, down)          # both parities, normal and subnormal codes
    assert any(abs(t) < 2.0 ** -6 for t in ties) and (np.abs(v) > 448).sum() >= 2 and np.abs(got).max() == 448
    assert np.isinf(x[0, 32:64]).sum() == 2 and sorted(mk.DECODE[q.view(torch.uint8).numpy()[0, 32:64]][np.isinf(x[0, 32:64])].tolist()) == [-448.0, 448.0]
    assert (x[0, 64:96] == 0).all() and int(e[0, 2]) == 0
    sub = x[0, 96:128]
    assert (np.abs(sub) < 2.0 ** -126).all() and np.count_nonzero(sub) > 16 and int(e[0, 3]) == 0 and np.count_nonzero(q.view(torch.uint8).numpy()[0, 96:128] & 0x7F) > 16
    places = mk.quant_nan_places(rows, K)
    assert len(places) >= 3 and all(0 <= r < rows and 0 <= c < K for r, c in places) and (0, 5) in places


# ------------------------------------------------------------------------------------------------ what the table holds
def test_the_table_holds_every_edge():
    cs, ws = mk.CASES, mk.WSC_CASES
    assert {c["M"] for c in cs} >= {1, 255, 256, 257, 300, 513} and {c["N"] for c in cs} >= {1, 7, 9, 200, 256, 257, 264, 520}
    assert {c["K"] for c in cs} >= {128, 256, 384, 1536, 8960}
    assert {c["lda"] for c in cs} == {"K", "K+16", "2K"} and {c["ldw"] for c in cs} == {"K", "K+64"} and {c["ldc"] for c in cs} == {"N8", "N8+8", "half"}
    tiles = lambda c: (-(-c["M"] // 256)) * (-(-c["N"] // 256))
    assert {9, 10} <= {tiles(c) for c in cs} and any(-(-c["N"] // 256) >= 16 and -(-c["M"] // 256) % 5 == 1 for c in cs)
    assert -(-mk.BY_NAME[mk.GM_CASE]["M"] // 256) == 3 and mk.GM_VALUES == (1, 3)
    wide = [c for c in cs if c["N"] == 1540 and c["M"] == 257]
    assert {c["epi"] for c in wide} == set(mk.EPI)
    assert any(c["gate"] and c["gate_f32"] for c in wide) and any(c["gate"] and not c["gate_f32"] for c in wide) and any(c["epi"] == "gate_res" and not c["gate"] for c in wide)
    assert any(c["res"] == "own" and mk.dims(c)["ldres"] != mk.dims(c)["ldc"] for c in wide) and any(c["res"] == "inplace" for c in wide)
    ffn2 = mk.BY_NAME["k8960_ffn2"]
    assert ffn2["K"] == 8960 and ffn2["gate"] and ffn2["res"] == "inplace"
    assert any(c["ldc"] == "half" and c["res"] == "inplace" for c in cs) and any(c["ldc"] == "half" and c["res"] is None for c in cs)
    assert {c["sc_extra"] for c in cs} == {0, 256} == {c["sc_extra"] for c in ws} and sum(c["a_front"] % 32 == 16 for c in cs) == 1
    for c in cs:          # the narrow N edges run the exact epilogues
        assert c["N"] >= 1536 or mk.exact_epilogue(c), c["name"]
    assert {c["M"] for c in ws} >= {1, 256, 257, 300} and {c["N"] for c in ws} >= {1, 255, 257, 300, 520} and {c["K"] for c in ws} >= {128, 384, 1536}
    assert {c["bias"] for c in ws} == {None, "m", "n"} and all(c["ldc"] == "N8+8" and c["wsc"] and c["epi"] == "bias" for c in ws)
    vt = mk.BY_NAME["w_vt"]
    assert (vt["M"], vt["N"], vt["bias"]) == (512, 297, "m")
    assert sum(mk.accumulation_only(c) for c in cs + ws) >= 8
    assert all(mk.BY_NAME[n]["M"] > mk.NAN_AT[0] > 256 and mk.BY_NAME[n]["N"] > mk.NAN_AT_W[0] and mk.BY_NAME[n]["K"] > max(mk.NAN_AT[1], mk.NAN_AT_W[1]) for n in mk.NAN_CASES)
