"""-m gpu: the MX-fp8 kernels of csrc/svi_gemm.hip element by element, in the strided forms the DiT launches them — gemm_mx8_nt_256_kernel<false>
(svi_gemm_mx8), gemm_mx8_nt_256_kernel<true> (svi_gemm_mx8_wscaled) and mx8_quantize_kernel (svi_mx8_quantize).

Cases, operands, arenas, references and the bound: tests/mx8_kernel_cases.py (held on the host by tests/test_mx8_kernel_cases.py).  Per GEMM launch the
whole allocation of C comes back; what the launch does not own keeps its bits; the owned part has no NaN (A8 / W8 lie in 0x7F bytes, the scale table
holds 0xFF in every row past the operand's, bias / gate / residual lie in NaN) and meets the per-element bound against the fp64 reference, with the
moved roundings of every row under the cap.  The grid operands make fp32 accumulation exact in any order, so the bound asks for the reference's bits
wherever the epilogue is exact; whether the device gave them in the accumulation-only cases is reported.  The identity / byte-table, scale-table and
NaN-byte tests compare exactly.  The quantiser is held bit for bit to oracle/mx8_oracle.py at ties, saturation, infinities, zero and subnormal blocks,
in NaN-padded strided arenas; a NaN element must leave as an e4m3 NaN byte."""
import functools
import itertools

import numpy as np
import pytest
import torch

import mx8_kernel_cases as mk
from gpu_util import report
from row_kernel_cases import FILL, GUARD_ROWS, MOVED_CAP

pytestmark = pytest.mark.gpu
TOTAL = dict(cases=set(), launches=0, bad=0, moved=0, worst_units=0.0, worst_row_share=0.0, acc_only=0, acc_only_exact=0, exact_epilogue=0, exact_epilogue_bits=0)


@pytest.fixture(scope="module")
def hip():
    import svi_hip
    assert svi_hip._lib.lib().svi_device_count() >= 1
    return svi_hip


def sync():
    """Drain the device; a launch that faulted ends the session here instead of letting later tests run on the same device."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error after an MX-fp8 launch: {e}", returncode=3)


@functools.lru_cache(maxsize=4)
def host_arenas(name):
    return mk.arenas(mk.BY_NAME[name])


def to_device(key, arr):
    if key in ("A8", "W8"):
        return torch.from_numpy(arr).cuda()
    if key == "SC":
        return torch.from_numpy(arr.view(np.int32)).cuda()
    return torch.from_numpy(arr.astype(np.float32)).to(device="cuda", dtype=torch.float32 if key == "gate" else torch.bfloat16)


class Device:
    """A case's allocations on the device (A8 / W8 bytes, SC dwords, gate fp32, the rest bf16) and the operands' pointers."""
    def __init__(self, case, host=None):
        self.case, self.t, self.off = case, {}, {}
        for key, (arr, off) in (host_arenas(case["name"]) if host is None else host).items():
            self.off[key], self.t[key] = off, to_device(key, arr)

    def p(self, key, extra=0):
        if key not in self.off:
            return None
        t = self.t[key]
        return t.data_ptr() + (self.off[key] + extra) * t.element_size()

    def res(self):
        return self.p("C" if self.case["res"] == "inplace" else "res") if self.case["res"] else None

    def bits(self, key="C"):
        sync()
        t = self.t[key]
        return (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy()

    def values(self):
        sync()
        return self.t["C"].float().cpu().numpy()


def launch(hip, dv, **over):
    """The case's launch through the C ABI (`over`: K, lda, sc_rows of a refusal); returns the status."""
    L, c, d = hip._lib, dv.case, dict(mk.dims(dv.case), K=dv.case["K"])
    d.update(over)
    M, N, st = c["M"], c["N"], L.current_stream()
    if c["wsc"]:
        return L.lib().svi_gemm_mx8_wscaled(dv.p("A8"), d["lda"], dv.p("W8"), d["ldw"], dv.p("SC"), d["sc_rows"], dv.p("C"), d["ldc"], M, N, d["K"], dv.p("bias"),
                                            1 if c["bias"] == "m" else 0, st)
    return L.lib().svi_gemm_mx8(dv.p("A8"), d["lda"], dv.p("SC"), d["sc_rows"], dv.p("W8"), d["ldw"], dv.p("C"), d["ldc"], M, N, d["K"], dv.p("bias"), mk.EPI[c["epi"]],
                                dv.p("gate"), dv.res(), d["ldres"], st)


def run(hip, name, host=None):
    dv = Device(mk.BY_NAME[name], host)
    st = launch(hip, dv)
    sync()
    assert st == 0, (name, st, hip._lib.last_error())
    return dv


def unowned_kept(name, dv, what=""):
    case = mk.BY_NAME[name]
    own, before = mk.owned(case), Device(case).bits()
    after = dv.bits()
    assert np.array_equal(after[~own], before[~own]), f"{name}{what}: the launch wrote {int((after[~own] != before[~own]).sum())} elements of C's allocation it does not own"


def check(name, dv, what="", ref=None):
    """The unowned part bit-equal, no NaN in the owned part, the bound and the cap; returns (owned block, whether it is the reference's bits)."""
    case, ref = mk.BY_NAME[name], mk.reference(name) if ref is None else ref
    unowned_kept(name, dv, what)
    got = mk.c_view(case, dv.values())
    assert not np.isnan(got).any(), f"{name}{what}: {int(np.isnan(got).sum())} NaN, first at {np.argwhere(np.isnan(got))[0].tolist()}"
    v = mk.verdict(got, ref["want"], ref["s"])
    exact = bool(np.array_equal(got.astype(np.float64), ref["want"]))
    with np.errstate(invalid="ignore", divide="ignore"):          # the accumulation's own difference, where nothing follows it: units of 2^-24 S0
        acc_units = float(np.where(got == ref["want"], 0.0, np.abs(got - ref["want"]) / (2.0 ** -24 * ref["s0"])).max()) if mk.accumulation_only(case) else None
    report("mx8_kernels", case=name + what, exact=exact, accumulation_only=mk.accumulation_only(case), acc_diff_units_of_s0=acc_units, **v)
    print(name + what, "exact" if exact else "NOT the reference's bits", v)
    TOTAL["cases"].add(name)
    TOTAL["launches"] += 1
    TOTAL["bad"] += v["bad"]
    TOTAL["moved"] += v["moved"]
    TOTAL["worst_units"] = max(TOTAL["worst_units"], v["worst_units"])
    TOTAL["worst_row_share"] = max(TOTAL["worst_row_share"], v["worst_row_share"])
    if mk.accumulation_only(case):
        TOTAL["acc_only"] += 1
        TOTAL["acc_only_exact"] += exact
    if mk.exact_epilogue(case):
        TOTAL["exact_epilogue"] += 1
        TOTAL["exact_epilogue_bits"] += exact
    assert v["bad"] == 0, (name, what, v)
    assert v["worst_row_share"] <= MOVED_CAP, (name, what, v)
    return got, exact


# ------------------------------------------------------------------------------------------------ both GEMMs, every case
@pytest.mark.parametrize("name", [c["name"] for c in mk.CASES])
def test_a_scaled_case(hip, name):
    check(name, run(hip, name))


@pytest.mark.parametrize("name", [c["name"] for c in mk.WSC_CASES])
def test_w_scaled_case(hip, name):
    """The bound, the mask, and — where svi_gemm_mx8 accepts the swapped problem (no bias along N) — its bits on the swapped operands, transposed."""
    case, d, L = mk.BY_NAME[name], mk.dims(mk.BY_NAME[name]), hip._lib
    dv = run(hip, name)
    check(name, dv)
    if case["bias"] != "n":
        M, N, K = case["M"], case["N"], case["K"]
        ld2 = (M + 7) // 8 * 8 + 8
        c2 = torch.full((N + GUARD_ROWS, ld2), FILL, dtype=torch.bfloat16, device="cuda")
        st = L.lib().svi_gemm_mx8(dv.p("W8"), d["ldw"], dv.p("SC"), d["sc_rows"], dv.p("A8"), d["lda"], c2.data_ptr(), ld2, N, M, K, dv.p("bias"), 0, None, None, 0, L.current_stream())
        sync()
        assert st == 0, (name, st, L.last_error())
        back = c2.view(torch.int16).cpu().numpy()
        own = mk.c_view(case, dv.bits())
        assert np.array_equal(back[:N, :M].T, own), (name, "differs from svi_gemm_mx8 on the swapped operands")
        assert (c2[N:].float() == FILL).all() and (c2[:, M:].float() == FILL).all()
        TOTAL["launches"] += 1


@pytest.mark.parametrize("gm", mk.GM_VALUES)
def test_group_height_switch(hip, gm):
    """Three row panels under SVI_GEMM_GM = 1 (three groups of one) and 3 (one group of three): the same bits as the launcher's own height 2."""
    name = mk.GM_CASE
    base = run(hip, name).bits()
    hip._lib.set_switch("SVI_GEMM_GM", gm)
    try:
        dv = run(hip, name)
    finally:
        hip._lib.set_switch("SVI_GEMM_GM", None)
    check(name, dv, f"@gm{gm}")
    assert np.array_equal(dv.bits(), base), (gm, "differs from the default group height")


# ------------------------------------------------------------------------------------------------ identity against every byte and every scale
@pytest.mark.parametrize("name", [c["name"] for c in mk.TABLE_CASES])
def test_byte_and_scale_tables(hip, name):
    """One operand the identity, the other every finite e4m3 code: C is the widened byte (times its block's scale), exactly; -0 may come out as +0."""
    case, want = mk.BY_NAME[name], mk.reference(name)["want"]
    dv = run(hip, name)
    unowned_kept(name, dv)
    got = mk.c_view(case, dv.values()).astype(np.float64)
    wrong = ~(got == want)          # (NaN compares unequal)
    report("mx8_kernels_table", case=name, wrong=int(wrong.sum()))
    TOTAL["launches"] += 1
    assert not wrong.any(), (name, int(wrong.sum()), "first at", np.argwhere(wrong)[0].tolist(), got[tuple(np.argwhere(wrong)[0])], want[tuple(np.argwhere(wrong)[0])])


@pytest.mark.parametrize("name,operand,byte", [(n, o, b) for n in mk.NAN_CASES for o, b in (("A8", 0x7F), ("A8", 0xFF), ("W8", 0x7F), ("W8", 0xFF))])
def test_a_nan_byte_makes_its_row_or_column_nan_and_nothing_else(hip, name, operand, byte):
    case, d, want = mk.BY_NAME[name], mk.dims(mk.BY_NAME[name]), mk.reference(name)["want"]
    host = dict(host_arenas(name))
    flat, off = host[operand]
    r, k = mk.NAN_AT if operand == "A8" else mk.NAN_AT_W
    flat = flat.copy()
    flat[off + r * d["lda" if operand == "A8" else "ldw"] + k] = byte
    host[operand] = (flat, off)
    dv = run(hip, name, host)
    unowned_kept(name, dv)
    got = mk.c_view(case, dv.values()).astype(np.float64)
    nan = np.isnan(got)
    expect = np.zeros_like(nan)
    if operand == "A8":
        expect[r] = True
    else:
        expect[:, r] = True
    TOTAL["launches"] += 1
    assert np.array_equal(nan, expect), (name, operand, hex(byte), int(nan.sum()), int(expect.sum()))
    assert np.array_equal(got[~nan], want[~nan])          # (exact epilogue, grid operands: everything else is the reference's bits)


def test_refusals_leave_c_untouched(hip):
    """K = 192, lda = K + 8 and a scale table that does not cover M: a status, a message, C as it was — for both entry points."""
    for name in ("m300", "w_m300"):
        case = mk.BY_NAME[name]
        for what, over, text in (("K = 192", dict(K=192), "multiple of 128"), ("lda = K + 8", dict(lda=case["K"] + 8), "bad leading dims"),
                                 ("sc_rows short", dict(sc_rows=mk.ceil256(case["N" if case["wsc"] else "M"]) - 256), "scale table must cover")):
            dv = Device(case)
            before = dv.bits().copy()
            st = launch(hip, dv, **over)
            sync()
            assert st != 0 and text in hip._lib.last_error(), (name, what, st, hip._lib.last_error())
            assert np.array_equal(dv.bits(), before), (name, what, "a refused launch wrote to C")


# ------------------------------------------------------------------------------------------------ the quantiser
Q_FILL, S_FILL = 0xA5, 0x5A5A5A5A
LDX, LDQ = ("K", "K+8", "2K"), ("K", "K+8", "K+64")


def _ld(kind, K):
    return {"K": K, "K+8": K + 8, "2K": 2 * K, "K+64": K + 64}[kind]


def quantize(L, x, ldx, ldq, sc_rows):
    """x [rows, K] fp64 of bf16 values -> (q bytes [rows + GUARD_ROWS, ldq] behind GUARD_FRONT bytes, scale dwords [K / 128 + 2, sc_rows]) as they come back:
    x lies in NaN (front, pad columns, rows after), q in Q_FILL, the table in S_FILL."""
    rows, K = x.shape
    xa = np.full((rows + GUARD_ROWS, ldx), np.nan, dtype=np.float32)
    xa[:rows, :K] = x
    xd = torch.from_numpy(np.concatenate([np.full(mk.GUARD_FRONT, np.nan, dtype=np.float32), xa.ravel()])).to(device="cuda", dtype=torch.bfloat16)
    qd = torch.full((mk.GUARD_FRONT + (rows + GUARD_ROWS) * ldq,), Q_FILL, dtype=torch.uint8, device="cuda")
    sd = torch.full((K // 128 + 2, sc_rows), S_FILL, dtype=torch.int32, device="cuda")
    st = L.lib().svi_mx8_quantize(xd.data_ptr() + 2 * mk.GUARD_FRONT, ldx, rows, K, qd.data_ptr() + mk.GUARD_FRONT, ldq, sd.data_ptr() + 4 * sc_rows, sc_rows, L.current_stream())
    sync()
    assert st == 0, (st, L.last_error())
    q = qd.cpu().numpy()
    assert (q[:mk.GUARD_FRONT] == Q_FILL).all(), "bytes written in front of q"
    return q[mk.GUARD_FRONT:].reshape(rows + GUARD_ROWS, ldq), sd.cpu().numpy().view(np.uint32)


def quant_unowned_kept(q, sc, rows, K):
    assert (q[rows:] == Q_FILL).all() and (q[:, K:] == Q_FILL).all(), "q: pad bytes or rows past the operand written"
    assert (sc[0] == S_FILL).all() and (sc[-1] == S_FILL).all() and (sc[:, rows:] == S_FILL).all(), "scale dwords of rows past the operand (or outside the table) written"


@pytest.mark.parametrize("rows,K", mk.QUANT_SHAPES)
def test_quantiser_bit_for_bit_in_strided_arenas(hip, rows, K):
    from oracle import mx8_oracle as mx
    L, x = hip._lib, mk.quant_input(rows, K)
    qo, eo = mx.mx8_quantize(torch.from_numpy(x).float())
    qo, want_sc = qo.view(torch.uint8).numpy(), mk.pack_scales(eo.numpy(), rows)
    n = 0
    for lx, lq, sc_rows in itertools.product(LDX, LDQ, (rows, mk.ceil256(rows), mk.ceil256(rows) + 256)):
        q, sc = quantize(L, x, _ld(lx, K), _ld(lq, K), sc_rows)
        diff = q[:rows, :K] != qo
        assert not diff.any(), (lx, lq, sc_rows, int(diff.sum()), "first at", np.argwhere(diff)[0].tolist())
        assert np.array_equal(sc[1:-1, :rows], want_sc), (lx, lq, sc_rows, "block scales differ")
        quant_unowned_kept(q, sc, rows, K)
        n += 1
    report("mx8_kernels_quantiser", rows=rows, K=K, launches=n, wrong_bytes=0)


@pytest.mark.parametrize("rows,K", mk.QUANT_SHAPES)
def test_quantiser_keeps_a_nan(hip, rows, K):
    """A NaN element leaves as an e4m3 NaN byte exactly where it stood; blocks without one are the oracle's bits.  (The scale code of a block that holds
    one is not compared: the oracle derives it from a NaN maximum, the kernel from the other elements.)"""
    from oracle import mx8_oracle as mx
    L, x = hip._lib, mk.quant_input(rows, K)
    qo, eo = mx.mx8_quantize(torch.from_numpy(x).float())
    qo, want_sc = qo.view(torch.uint8).numpy(), eo.numpy()
    places = mk.quant_nan_places(rows, K)
    xn = x.copy()
    for r, c in places:
        xn[r, c] = np.nan
    q, sc = quantize(L, xn, K + 8, K + 64, mk.ceil256(rows) + 256)
    is_nan = (q[:rows, :K] & 0x7F) == 0x7F
    expect = np.isnan(xn)
    report("mx8_kernels_quantiser_nan", rows=rows, K=K, planted=len(places), nan_bytes=int(is_nan.sum()), kept=int((is_nan & expect).sum()))
    assert np.array_equal(is_nan, expect), (places, np.argwhere(is_nan).tolist(), [hex(q[r, c]) for r, c in places])
    clean = np.repeat(~expect.reshape(rows, K // 32, 32).any(-1), 32, axis=1)
    assert np.array_equal(q[:rows, :K][clean], qo[clean])
    codes = np.stack([(sc[1:-1, :rows] >> (8 * b)) & 0xFF for b in range(4)], axis=-1).transpose(1, 0, 2).reshape(rows, K // 32)
    assert np.array_equal(codes[clean[:, ::32]], want_sc[clean[:, ::32]])
    quant_unowned_kept(q, sc, rows, K)


def test_quantiser_into_gemm_through_the_dit_seam(hip):
    """svi_mx8_quantize writes A8 and its scale table into the poisoned arenas of the case (lda > K, sc_rows beyond the tile rounding, 0xFF in every row it
    does not own); svi_gemm_mx8 on them equals the reference computed from the oracle's quantisation."""
    name, L = mk.SEAM["name"], hip._lib
    case, d, ops = mk.SEAM, mk.dims(mk.SEAM), mk.operands(mk.SEAM["name"])
    host = dict(host_arenas(name))
    blank = dict(host)
    for key in ("A8", "SC"):          # the operand itself blanked out: what the GEMM reads there is what the quantiser wrote
        flat, off = host[key]
        blank[key] = (np.full_like(flat, 0x7F if key == "A8" else 0xFFFFFFFF), off)
    dv = Device(case, blank)
    xd = torch.from_numpy(ops["x"].astype(np.float32)).to(device="cuda", dtype=torch.bfloat16).contiguous()
    st = L.lib().svi_mx8_quantize(xd.data_ptr(), case["K"], case["M"], case["K"], dv.p("A8"), d["lda"], dv.p("SC"), d["sc_rows"], L.current_stream())
    sync()
    assert st == 0, L.last_error()
    assert np.array_equal(dv.bits("A8"), host["A8"][0]) and np.array_equal(dv.bits("SC").view(np.uint32), host["SC"][0]), "the quantiser's arenas differ from the oracle's"
    st = launch(hip, dv)
    sync()
    assert st == 0, L.last_error()
    check(name, dv)


def test_totals(hip):
    """The figures of this file's GEMM launches in one report line (profiles/mx8_kernels_parity.txt is written from it)."""
    t = dict(TOTAL, cases=len(TOTAL["cases"]))
    report("mx8_kernels_totals", **t)
    print(t)
    assert t["bad"] == 0
