"""-m gpu: the bf16 GEMM kernels of csrc/svi_gemm.hip, element by element, in the strided forms the DiT launches them.

Cases, arenas, references and the bound: tests/gemm_kernel_cases.py (held on the host by tests/test_gemm_kernel_cases.py).  Every case runs on every
kernel path whose preconditions it meets — the 128^2 tile with one K tile of loads in flight, with four on four waves, with four on eight waves, the
256 x 192 tile, the 256^2 tile with four and with two phases per K tile — selected with SVI_GEMM_KERNEL / SVI_GEMM_PF and confirmed through
svi_gemm_plan.  Per launch: the whole allocation of C comes back; what the launch does not own (pad columns [N, ldc), rows past M, the other half of a
two-projection buffer, the elements before C) holds the bits it held; the owned part has no NaN (A, W, the residual, bias and gate are surrounded by
NaN: a read outside an operand that reaches an output shows) and meets the per-element bound with the moved roundings of every row under the cap;
and it is bit for bit what the one-in-flight 128^2 kernel gives.  svi_gemm_bf16_pair (the q | k launch: W2 / bias2 / n_split, and sel_m / sel_n) is
held to the same and to two svi_gemm_bf16 launches on the halves."""
import functools

import numpy as np
import pytest
import torch

import gemm_kernel_cases as gk
from gpu_util import report
from row_kernel_cases import FILL, MOVED_CAP

pytestmark = pytest.mark.gpu
EPS = 1e-6


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
        pytest.exit(f"device error after a GEMM launch: {e}", returncode=3)


class on_path:
    """SVI_GEMM_KERNEL / SVI_GEMM_PF of a path for the duration (None: the launcher's own choice)."""
    def __init__(self, hip, path):
        self.L, self.path = hip._lib, path

    def __enter__(self):
        if self.path is not None:
            kind, pf = gk.PATHS[self.path]
            self.L.set_switch("SVI_GEMM_KERNEL", kind)
            self.L.set_switch("SVI_GEMM_PF", pf)

    def __exit__(self, *exc):
        self.L.set_switch("SVI_GEMM_KERNEL", None)
        self.L.set_switch("SVI_GEMM_PF", None)


@functools.lru_cache(maxsize=8)
def host_arenas(name):
    return gk.arenas(gk.BY_NAME[name])


class Device:
    """A case's allocations on the device: bf16 (gate, ss, rs: fp32), and the operands' pointers."""
    def __init__(self, case):
        self.case, self.t, self.off = case, {}, {}
        for key, (arr, off) in host_arenas(case["name"]).items():
            self.off[key] = off
            if arr is not None:
                f32 = key in ("gate", "ss")
                self.t[key] = torch.from_numpy(arr.astype(np.float32)).to(device="cuda", dtype=torch.float32 if f32 else torch.bfloat16)
        if case["stats"]:
            self.t["rs"] = torch.full((case["M"] + gk.GUARD_FRONT,), FILL, dtype=torch.float32, device="cuda")

    def p(self, key, extra=0):
        if key not in self.off:
            return None
        t = self.t["W" if key == "W2" else key]
        return t.data_ptr() + (self.off[key] + extra) * t.element_size()

    def res(self, extra=0):
        return self.p("C" if self.case["res"] == "inplace" else "res", extra) if self.case["res"] else None

    def bits(self, key="C"):
        sync()
        t = self.t[key]
        return (t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)).cpu().numpy()

    def values(self, key="C"):
        sync()
        return self.t[key].float().cpu().numpy()


def launch(hip, dv, halves=False, sel=True, n_split=None, bias_along_m=None):
    """The case's launch through the C ABI (halves: two svi_gemm_bf16 launches on the column halves of a pair); returns the status."""
    L, c, d = hip._lib, dv.case, gk.dims(dv.case)
    M, N, K, st = c["M"], c["N"], c["K"], L.current_stream()
    ns = c["n_split"] if n_split is None else n_split
    along_m = (1 if c["bias"] == "m" else 0) if bias_along_m is None else bias_along_m
    common = (gk.EPI[c["epi"]],)
    if c["stats"]:
        return L.lib().svi_linear_row_stats(dv.p("A"), d["lda"], dv.p("W"), d["ldw"], dv.p("C"), d["ldc"], M, N, K, dv.p("bias"), EPS, dv.p("ss"), d["ldss"],
                                            dv.t["rs"].data_ptr(), st)
    if halves:
        s = L.lib().svi_gemm_bf16(dv.p("A"), d["lda"], dv.p("W"), d["ldw"], dv.p("C"), d["ldc"], M, ns, K, dv.p("bias"), along_m, *common,
                                  dv.p("gate"), dv.res(), d["ldres"], st)
        return s or L.lib().svi_gemm_bf16(dv.p("A"), d["lda"], dv.p("W2"), d["ldw"], dv.p("C", ns), d["ldc"], M, N - ns, K, dv.p("bias2"), along_m, *common,
                                          dv.p("gate", ns), dv.res(ns), d["ldres"], st)
    if c["n_split"] or c["sel_m"] or c["sel_n"]:
        return L.lib().svi_gemm_bf16_pair(dv.p("A"), d["lda"], dv.p("W"), d["ldw"], dv.p("C"), d["ldc"], M, N, K, dv.p("bias"), along_m, *common,
                                          dv.p("gate"), dv.res(), d["ldres"], dv.p("W2"), dv.p("bias2"), ns, c["sel_m"] if sel else 0, c["sel_n"] if sel else 0, st)
    return L.lib().svi_gemm_bf16(dv.p("A"), d["lda"], dv.p("W"), d["ldw"], dv.p("C"), d["ldc"], M, N, K, dv.p("bias"), along_m, *common,
                                 dv.p("gate"), dv.res(), d["ldres"], st)


def run(hip, name, path, **kw):
    """A fresh copy of the case's allocations, one launch on `path`: the device object after it."""
    dv = Device(gk.BY_NAME[name])
    with on_path(hip, path):
        st = launch(hip, dv, **kw)
    sync()
    assert st == 0, (name, path, st, hip._lib.last_error())
    return dv


def check(name, path, dv, what="gemm_kernels"):
    """Steps 4-6 of a case: the unowned part bit-equal, no NaN in the owned part, the bound and the cap."""
    case, ref = gk.BY_NAME[name], gk.reference(name)
    before = Device(case)
    own = gk.owned(case)
    b0, b1 = before.bits(), dv.bits()
    assert np.array_equal(b1[~own], b0[~own]), f"{name} on {path}: the launch wrote {int((b1[~own] != b0[~own]).sum())} elements of C's allocation it does not own"
    got = gk.c_view(case, dv.values())
    assert not np.isnan(got).any(), f"{name} on {path}: {int(np.isnan(got).sum())} NaN, first at {np.argwhere(np.isnan(got))[0].tolist()}"
    v = gk.verdict(got, ref["want"], ref["s"])
    report(what, case=name, path=path, **v)
    print(name, path, v)
    assert v["bad"] == 0, (name, path, v)
    assert v["worst_row_share"] <= MOVED_CAP, (name, path, v)
    return got


_first = {}          # case -> the owned bits (and statistics) of the one-in-flight 128^2 kernel


def baseline(hip, name):
    if name not in _first:
        dv = run(hip, name, "t128_pf1")
        _first[name] = (dv.bits(), dv.bits("ss") if gk.BY_NAME[name]["stats"] else None, dv.bits("rs") if gk.BY_NAME[name]["stats"] else None)
    return _first[name]


# ------------------------------------------------------------------------------------------------ the case table x kernel path
@pytest.mark.parametrize("name,path", [(c["name"], p) for c in gk.CASES for p in gk.PATHS if gk.applies(c, p)])
def test_case_on_path(hip, name, path):
    case, L = gk.BY_NAME[name], hip._lib
    with on_path(hip, path):
        assert L.gemm_plan(case["M"], case["N"], case["K"], gk.EPI[case["epi"]], compute_units=256) == gk.PATHS[path][0]
    dv = run(hip, name, path)
    got = check(name, path, dv)
    first = baseline(hip, name)
    assert np.array_equal(dv.bits(), first[0]), (name, path, "differs from the one-in-flight 128^2 kernel")
    if case["stats"]:
        own = gk.owned_ss(case)
        ss_bits = dv.bits("ss")
        assert (dv.values("ss")[~own] == np.float32(FILL)).all(), (name, path, "row statistics written outside [N / 64, M]")
        assert np.array_equal(ss_bits, first[1]) and np.array_equal(dv.bits("rs"), first[2]), (name, path, "row statistics differ between kernels")
        ss = gk.ss_view(case, dv.values("ss")).astype(np.float64)
        want_ss = (got.astype(np.float64) ** 2).reshape(case["M"], case["N"] // 64, 64).sum(-1).T          # fp64, of the rounded output that came back
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where(want_ss == 0, np.abs(ss), np.abs(ss - want_ss) / want_ss)
        rs = dv.values("rs")
        want_rs = 1.0 / np.sqrt(want_ss.sum(0) / case["N"] + EPS)
        rel_rs = float(np.linalg.norm(rs[:case["M"]] - want_rs) / np.linalg.norm(want_rs))
        report("gemm_kernels_row_stats", case=name, path=path, worst_rel_sumsq=float(rel.max()), rel_rs=rel_rs)
        assert rel.max() <= 1e-6 and rel_rs <= 1e-6, (name, path, float(rel.max()), rel_rs)
        assert (rs[case["M"]:] == np.float32(FILL)).all()


# ------------------------------------------------------------------------------------------------ svi_gemm_bf16_pair
@pytest.mark.parametrize("name,path", [(c["name"], p) for c in gk.PAIR_CASES for p in gk.PATHS if gk.applies(c, p)])
def test_pair_launch_on_path(hip, name, path):
    """One launch with the moved W base where n_split is a multiple of the path's tile width, two launches where it is not: the bound, the mask, and the
    bits of two svi_gemm_bf16 launches on the halves (and of the one-in-flight 128^2 kernel)."""
    dv = run(hip, name, path)
    check(name, path, dv, "gemm_kernels_pair")
    assert np.array_equal(dv.bits(), run(hip, name, path, halves=True).bits()), (name, path, "differs from two launches on the halves")
    assert np.array_equal(dv.bits(), baseline(hip, name)[0]), (name, path)


def test_pair_launch_refuses_what_it_cannot_serve(hip):
    """Each of these returns a non-zero status with its message and leaves C's allocation as it was."""
    name = "pair_s200"
    N = gk.BY_NAME[name]["N"]
    for what, kw, text in (("n_split not a multiple of 8", dict(n_split=100), "multiple of 8"), ("n_split = 0", dict(n_split=0), "bad weight pair"),
                           ("n_split = N", dict(n_split=N), "bad weight pair"), ("bias along M", dict(bias_along_m=1), "bad weight pair")):
        for path in ("t128_pf1", "t256_ph2"):
            dv = Device(gk.BY_NAME[name])
            before = dv.bits().copy()
            with on_path(hip, path):
                st = launch(hip, dv, **kw)
            sync()
            assert st != 0 and text in hip._lib.last_error(), (what, path, st, hip._lib.last_error())
            assert np.array_equal(dv.bits(), before), (what, path, "a refused launch wrote to C")


@pytest.mark.parametrize("name", [c["name"] for c in gk.SEL_CASES])
def test_stacked_launch_keeps_the_per_sample_kernel(hip, name):
    """No switch set.  sel_m: two samples of L rows stacked — with sel_m = L the bits of the two per-sample launches; sel_n: q | k side by side — with
    sel_n = D the bits of the two per-projection launches.  Without the override the launcher takes a 256-row kernel: the bound still holds."""
    case, L, d = gk.BY_NAME[name], hip._lib, gk.dims(gk.BY_NAME[name])
    M, N, K = case["M"], case["N"], case["K"]
    with on_path(hip, None):
        assert L.gemm_plan(M, N, K, compute_units=256) in (192, 259, 260)
        assert L.gemm_plan(case["sel_m"] or M, case["sel_n"] or N, K, compute_units=256) == 128
    chosen = run(hip, name, None)
    check(name, "sel", chosen, "gemm_kernels_sel")
    check(name, "auto", run(hip, name, None, sel=False), "gemm_kernels_sel")
    if case["sel_n"]:
        parts = run(hip, name, None, halves=True)
    else:
        parts = Device(case)
        h = case["sel_m"]
        for r0 in (0, h):
            st = L.lib().svi_gemm_bf16(parts.p("A", r0 * d["lda"]), d["lda"], parts.p("W"), d["ldw"], parts.p("C", r0 * d["ldc"]), d["ldc"], h, N, K,
                                       parts.p("bias"), 0, gk.EPI[case["epi"]], None, None, 0, L.current_stream())
            assert st == 0, L.last_error()
    assert np.array_equal(chosen.bits(), parts.bits()), (name, "the stacked launch differs from its per-sample launches")
