"""The case table, references, bound and write mask of the GEMM kernel GPU tests (tests/gemm_kernel_cases.py), checked on the host: the fp32
emulation meets the per-element bound against the fp64 reference with zero failures and its moved roundings under the cap in every row; the figures
the module's docstring states are the ones measured; every planted fault is caught; arenas, masks and NaN placement agree for every case; the table
holds every edge the GPU file is about; and the planner facts the sel_m / sel_n cases rest on hold."""
import collections
import json

import numpy as np
import pytest

import gemm_kernel_cases as gk
from row_kernel_cases import FILL, GUARD_ROWS, MOVED_CAP, rbf32, rbf64

TABLE = [c["name"] for c in gk.CASES + gk.PAIR_CASES]
_seen = {}


def _emulated(name):
    """(reference, emulation, verdict, noise) of a case's own inputs, once."""
    if name not in _seen:
        ref, emu = gk.reference(name), gk.emulation(name)
        _seen[name] = (ref, emu, gk.verdict(emu["out"], ref["want"], ref["s"]), gk.noise_units(ref, emu))
    return _seen[name]


@pytest.mark.parametrize("name", TABLE)
def test_emulation_meets_the_bound(name):
    ref, emu, v, noise = _emulated(name)
    print(json.dumps({"test": "gemm_emulation", "case": name, "noise_acc": noise[0], "noise_last": noise[1], **v}))
    assert v["bad"] == 0, v
    assert v["worst_row_share"] < MOVED_CAP, v
    assert max(noise) <= gk.C_NOISE / 2, noise          # C_NOISE is the measured power of two, doubled once
    assert np.isfinite(ref["want"]).all() and np.abs(ref["want"]).max() < 2.0 ** 100          # every output finite in bf16, the 2^80 element included
    assert np.array_equal(rbf64(ref["want"]), ref["want"])
    if gk.BY_NAME[name]["epi"] in ("bias", "relu") or (gk.BY_NAME[name]["epi"] == "gate_res" and not gk.BY_NAME[name]["gate_f32"]):
        assert v["moved"] == 0 and np.array_equal(emu["out"].astype(np.float64), ref["want"]), v          # exact arithmetic: the reference's bits


def test_noise_constant_and_moved_share_as_documented():
    worst_acc = max(_emulated(n)[3][0] for n in TABLE)
    worst_last = max(_emulated(n)[3][1] for n in TABLE)
    worst_share = max(_emulated(n)[2]["worst_row_share"] for n in TABLE)
    print(worst_acc, worst_last, worst_share)
    assert worst_acc <= 0.03 and 1.0 < worst_last <= 1.41 + 1e-2 and worst_share <= 1.3e-3 + 1e-5
    assert gk.C_NOISE == 4.0 and MOVED_CAP == 2e-3
    doc = gk.__doc__
    assert "C_NOISE = 4" in doc and "1.41 units" in doc and "1.3e-3" in doc and "seeds {per-case default, 1, 2,\n3}" in doc


def test_the_bound_sorts_equal_moved_and_wrong():
    want = np.array([[1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 1.9921875]])
    got = np.array([[1.0, 1.0078125, 1.015625, 1.0234375, 0.0, 1e-30, 2.0]])
    moved, bad, _ = gk.judge(got, want, np.abs(want))
    assert moved.tolist() == [[False, True, True, False, False, False, True]]          # without cancellation only equality meets the bound
    assert bad.tolist() == [[False, False, False, True, False, True, False]]
    # a cancelling residual: noise and window are relative to S
    w3 = np.full((1, 3), 0.0078125)
    moved, bad, _ = gk.judge(w3 + np.array([[2.0 ** -23, 2.0 ** -8, 2.0 ** -4]]), w3, np.full((1, 3), 2.0))
    assert moved.tolist() == [[False, True, False]] and bad.tolist() == [[False, False, True]]
    assert gk.judge(np.array([[np.nan, np.inf]]), np.ones((1, 2)), np.ones((1, 2)))[1].all()


# ------------------------------------------------------------------------------------------------ planted faults
MUTANTS = {          # fault -> a case on which it must show
    "bias_transposed": ("m300_n392", "s_vt", "wide_gelu_erf"),
    "gate_after_res": ("m300_n392", "k1536", "wide_gate_f32"),
    "no_y1_rounding": ("wide_gelu_tanh", "m300_n392", "k128"),
    "swap_columns": ("n9", "wide_bias", "pair_s200"),
}


@pytest.mark.parametrize("fault", sorted(MUTANTS))
def test_planted_faults_fail_the_bound(fault):
    for name in MUTANTS[fault]:
        ref = gk.reference(name)
        v = gk.verdict(gk.emulation(name, mutate=fault)["out"], ref["want"], ref["s"])
        assert v["bad"] > 0 or v["worst_row_share"] > MOVED_CAP, (fault, name, v)
        assert _emulated(name)[2]["bad"] == 0


def test_an_element_written_into_a_pad_column_fails_the_mask():
    for name in ("n193", "m257", "s_half_inplace", "k8"):
        case = gk.BY_NAME[name]
        d, before = gk.dims(case), gk.arenas(case)["C"][0]
        after, own = gk.expected_c(case, gk.reference(name)["want"]), gk.owned(case)
        assert np.array_equal(after[~own], before[~own]) and not np.array_equal(after[own], before[own])
        grid = after[gk.GUARD_FRONT:].reshape(case["M"] + GUARD_ROWS, d["ldc"])
        for r, c in ((0, d["c_off"] + case["N"]), (case["M"], d["c_off"]), (0, d["c_off"] - 1)):          # pad column, row past M, the other half
            if 0 <= c < d["ldc"]:
                spoiled = grid.copy()
                spoiled[r, c] = 1.0
                assert not np.array_equal(np.concatenate([after[:gk.GUARD_FRONT], spoiled.ravel()])[~own], before[~own]), (name, r, c)
        spoiled = after.copy()
        spoiled[gk.GUARD_FRONT - 1] = 1.0          # the element before C
        assert not np.array_equal(spoiled[~own], before[~own])


# ------------------------------------------------------------------------------------------------ arenas, masks, NaN placement
@pytest.mark.parametrize("name", TABLE + [c["name"] for c in gk.SEL_CASES])
def test_arenas_masks_and_reference_shapes_agree(name):
    case, d = gk.BY_NAME[name], gk.dims(gk.BY_NAME[name])
    M, N, K, ns = case["M"], case["N"], case["K"], case["n_split"]
    ar = gk.arenas(case)
    a, w, bias, gate, res = gk.logical(case)
    for v in (a, w, bias, gate, res):
        if v is not None and not (v is gate and case["gate_f32"]):
            assert np.array_equal(rbf32(v.astype(np.float32)).astype(np.float64), v)          # bf16 values
    # the launcher's own requirements: strides multiples of 8 and wide enough, operands 16-byte aligned
    assert d["lda"] % 8 == 0 and d["ldw"] % 8 == 0 and d["ldc"] % 8 == 0 and d["ldres"] % 8 == 0 and d["lda"] >= K and d["ldw"] >= K and d["ldc"] >= d["c_off"] + N
    for key in ("A", "W", "C", "res", "W2"):
        if key in ar:
            assert ar[key][1] % 8 == 0, key

    def block(key, rows, ld, width, arr=None):
        flat, off = ar[key] if arr is None else (arr, ar[key][1])
        return np.stack([flat[off + r * ld: off + r * ld + width] for r in range(rows)])
    # the operand blocks are where the offsets say, and everything else of A / W / res / bias / gate is NaN
    assert np.array_equal(block("A", M, d["lda"], K), a)
    w_flat = ar["W"][0]
    n_w = ns if ns else N
    assert np.array_equal(block("W", n_w, d["ldw"], K), w[:n_w])
    finite = M * K
    assert np.isfinite(ar["A"][0]).sum() == finite and np.isnan(ar["A"][0][:gk.GUARD_FRONT]).all() and np.isnan(ar["A"][0][-GUARD_ROWS * d["lda"]:]).all()
    if ns:
        assert np.array_equal(block("W2", N - ns, d["ldw"], K, w_flat), w[ns:])
        assert ar["W2"][1] < ar["W"][1]                                                    # W2 lies before W ...
        moved_base = ar["W2"][1] - ns * d["ldw"]
        assert moved_base >= gk.GUARD_FRONT and np.isnan(w_flat[moved_base: ar["W2"][1]]).all()          # ... and the moved base inside the allocation, on NaN
        assert moved_base + (N - 1) * d["ldw"] + K <= len(w_flat)
    assert np.isfinite(w_flat).sum() == N * K
    if d["lda"] > K:
        assert np.isnan(block("A", M, d["lda"], d["lda"])[:, K:]).all()
    if "res" in ar:
        assert np.array_equal(block("res", M, d["ldres"], N), res) and np.isfinite(ar["res"][0]).sum() == M * N
    for key, vec in (("bias", bias), ("gate", gate)):
        if key in ar and not ns:
            flat, off = ar[key]
            assert np.array_equal(flat[off: off + len(vec)], vec) and np.isfinite(flat).sum() == len(vec) and (off % 8 == 1) == case["misalign"]
    if ns and bias is not None:
        assert np.array_equal(ar["bias"][0][ar["bias"][1]:][:ns], bias[:ns]) and np.array_equal(ar["bias2"][0][ar["bias2"][1]:][:N - ns], bias[ns:])
    # C: FILL outside the owned block (the residual inside it when in place); mask, view and reference shape agree
    c_flat, c_off = ar["C"]
    own = gk.owned(case)
    assert own.shape == c_flat.shape and own.sum() == M * N and (c_flat[~own] == FILL).all() and own[c_off] and not own[c_off - 1]
    assert gk.c_view(case, c_flat).shape == (M, N) and gk.c_view(case, own).all()
    if case["res"] == "inplace":
        assert np.array_equal(gk.c_view(case, c_flat), res)
    if name in TABLE:
        ref = gk.reference(name)
        assert ref["want"].shape == ref["s"].shape == (M, N)
        if case["stats"]:
            assert ref["ss"].shape == (N // 64, M) and gk.owned_ss(case).sum() == (N // 64) * M and d["ldss"] > M and N % 64 == 0 and d["ldc"] == 2 * N


@pytest.mark.parametrize("name", ["m300_n392", "n264_misaligned", "s_half_inplace", "pair_s192", "k136", "wide_gate_f32"])
def test_a_nan_inside_an_operand_arrives_and_one_outside_does_not(name):
    """The references read the logical operands, i.e. exactly [0, K) of each row and [0, N) of bias / gate: a NaN planted INSIDE an operand reaches the
    row / column it belongs to and nothing else."""
    case = gk.BY_NAME[name]
    a, w, bias, gate, res = gk.logical(case)
    M, N, K = case["M"], case["N"], case["K"]
    a2 = a.copy(); a2[M // 2, K - 1] = np.nan
    got = gk.reference_arrays(case, a2, w, bias, gate, res)["want"]
    assert np.isnan(got[M // 2]).all() and np.isfinite(np.delete(got, M // 2, axis=0)).all()
    w2 = w.copy(); w2[N - 2, 0] = np.nan
    got = gk.emulate_arrays(case, a, w2, bias, gate, res)["out"]
    assert np.isnan(got[:, N - 2]).all() and np.isfinite(np.delete(got, N - 2, axis=1)).all()
    if gate is not None:
        g2 = gate.copy(); g2[N - 1] = np.nan
        got = gk.reference_arrays(case, a, w, bias, g2, res)["want"]
        assert np.isnan(got[:, N - 1]).all() and np.isfinite(got[:, :N - 1]).all()


# ------------------------------------------------------------------------------------------------ what the table holds
def test_the_table_holds_every_edge():
    cs = gk.CASES
    assert {c["M"] for c in cs} >= {1, 127, 129, 255, 257, 300}
    assert {c["N"] for c in cs} >= {1, 7, 9, 191, 193, 200, 257, 264, 392}
    assert {c["K"] for c in cs} >= {64, 128, 256, 448, 1536, 8, 56, 72, 136}
    assert {c["lda"] for c in cs} == {"K", "K+8", "2K"} and {c["ldw"] for c in cs} == {"K", "K+64"} and {c["ldc"] for c in cs} == {"N8", "N8+8", "2N8", "half"}
    assert {c["epi"] for c in cs} == set(gk.EPI)
    assert any(c["res"] == "own" and gk.dims(c)["ldres"] != gk.dims(c)["ldc"] for c in cs) and any(c["res"] == "inplace" for c in cs)
    assert any(c["ldc"] == "half" and c["res"] == "inplace" for c in cs) and any(c["ldc"] == "half" and c["res"] == "own" for c in cs)
    assert any(c["epi"] == "gate_res" and not c["gate"] for c in cs) and any(c["bias"] is None for c in cs) and any(c["bias"] == "m" and c["epi"] == "bias" for c in cs)
    for epi in gk.EPI:          # every epilogue reaches every path, the 256-row kernels with an interior tile (M >= 256 and N >= 256)
        for path in gk.PATHS:
            assert any(c["epi"] == epi and gk.applies(c, path) and c["M"] >= 256 and c["N"] >= 256 for c in cs), (epi, path)
    for k in (8, 56, 72, 136):
        assert [p for p in gk.PATHS if gk.applies(dict(K=k, N=200), p)] == ["t128_pf1"]
    assert all(gk.applies(dict(K=256, N=192), p) for p in gk.PATHS) and not gk.applies(dict(K=192, N=200), "t128_pf8") and not gk.applies(dict(K=256, N=191), "t192")
    for c in gk.PAIR_CASES:
        assert c["ldc"] == "N8+8" and c["N"] % 8 == 0 and c["n_split"] % 8 == 0
    for path, tw in gk.TILE_WIDTH.items():          # per kernel: a split on its tile width (one launch) and one off it (two launches)
        assert any(c["n_split"] % tw == 0 and gk.applies(c, path) for c in gk.PAIR_CASES) and any(c["n_split"] % tw for c in gk.PAIR_CASES)
    assert any(c["gate"] and c["res"] for c in gk.PAIR_CASES if c["n_split"] % 128 == 0) and any(c["gate"] and c["res"] for c in gk.PAIR_CASES if c["n_split"] % 128)
    count = collections.Counter(p for _, p in gk.launches())
    assert (len(gk.CASES), len(gk.PAIR_CASES)) == (44, 6)
    assert count == {"t128_pf1": 50, "t128_pf4": 43, "t128_pf8": 43, "t192": 39, "t256_ph4": 45, "t256_ph2": 45} and "265 launches" in gk.__doc__


def test_edge_rows_are_in_the_inputs():
    a, w, bias, gate, res = gk.logical(gk.BY_NAME["m300_n392"])          # bias along N: W carries the 2^40 row
    assert (a[1] == 0).all() and 0 < np.abs(a[2]).max() <= 2.0 ** -38 and np.abs(a[-1]).max() <= 4 and (w[1] == 0).all() and np.abs(w[-1]).max() >= 2.0 ** 37 and bias[-1] == 0
    ref = gk.reference("m300_n392")
    t = rbf64(gate * ref["y1"][gk.CANCEL_ROW])
    assert (ref["want"][gk.CANCEL_ROW, 0::2] == 0).all() and (np.abs(ref["raw"][gk.CANCEL_ROW, 1::2]) <= 2.0 ** -4 * np.abs(t[1::2])).all()
    a, w, *_ = gk.logical(gk.BY_NAME["m300"])                            # no bias: both, meeting in one element of 2^80
    assert np.abs(a[-1]).max() >= 2.0 ** 37 and np.abs(w[-1]).max() >= 2.0 ** 37 and 2.0 ** 70 < abs(gk.reference("m300")["want"][-1, -1]) < 2.0 ** 100
    a, w, bias, *_ = gk.logical(gk.BY_NAME["m257"])                      # bias along M: A carries it
    assert np.abs(a[-1]).max() >= 2.0 ** 37 and np.abs(w[-1]).max() <= 4 and bias[-1] == 0


# ------------------------------------------------------------------------------------------------ the planner facts of the sel cases
def test_planner_facts_of_the_stacked_cases():
    from svi_hip import _lib as L
    for k in ("SVI_GEMM_KERNEL", "SVI_GEMM_PF"):
        L.set_switch(k, None)
    Lr, D, K = gk.SEL_L, gk.SEL_D, gk.SEL_K
    assert L.gemm_plan(2 * Lr, D, K, compute_units=256) in (192, 259, 260) and L.gemm_plan(Lr, D, K, compute_units=256) == 128          # stacked rows
    assert L.gemm_plan(Lr, 2 * D, K, compute_units=256) in (192, 259, 260)                                                         # stacked columns
    sm, sn = gk.BY_NAME["sel_m"], gk.BY_NAME["sel_n"]
    assert (sm["M"], sm["N"], sm["K"], sm["sel_m"]) == (2 * Lr, D, K, Lr) and (sn["M"], sn["N"], sn["n_split"], sn["sel_n"]) == (Lr, 2 * D, D, D)
    try:          # what confirms a path's kernel in the GPU file: the planner follows SVI_GEMM_KERNEL where the preconditions hold
        for path, (kind, _) in gk.PATHS.items():
            L.set_switch("SVI_GEMM_KERNEL", kind)
            for c in gk.CASES:
                if gk.applies(c, path):
                    assert L.gemm_plan(c["M"], c["N"], c["K"], gk.EPI[c["epi"]], compute_units=256) == kind, (c["name"], path)
                elif kind != 128:
                    assert L.gemm_plan(c["M"], c["N"], c["K"], gk.EPI[c["epi"]], compute_units=256) != kind, (c["name"], path)
    finally:
        L.set_switch("SVI_GEMM_KERNEL", None)
