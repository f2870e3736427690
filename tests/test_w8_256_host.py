"""SVI_GEMM_W8_256 without a GPU: what the e4m3 launch planner answers with the switch on and off, and the code object of the kernel it names
(gemm_w8_nt_256e_kernel, csrc/svi_gemm.hip: the two-phase 256^2 loop on the stored e4m3 bytes)."""
import itertools

from svi_hip import _lib as L
from test_code_objects import kernel_table
from test_fp8_resident_host import w8_plan

SWEEP = list(itertools.product((1, 16, 128, 129, 2560, 32760), (8, 136, 1536, 5120, 8960), (64, 72, 128, 1536, 8960), (0, 1, 2), (False, True)))


def today(b):
    """svi_gemm_w8_plan with the switch unset, from svi_gemm_plan's answer (tests/test_fp8_resident_host.py pins it)."""
    return b if b in (0, 128) else 128


def test_switch_moves_the_256_row_launches_to_260_and_nothing_else():
    try:
        L.set_switch("SVI_GEMM_W8_256", 1)
        moved = 0
        for M, N, K, epi, skinny in SWEEP:
            b, w = L.gemm_plan(M, N, K, epi, skinny=skinny), w8_plan(M, N, K, epi, skinny)
            assert w == (260 if b in (192, 259, 260) else today(b)), (M, N, K, epi, skinny, b, w)
            moved += w == 260
        assert moved > 0          # the sweep reaches the 256-row tiles
        for forced in (192, 259, 260):          # every id the bf16 planner can name for a 256-row tile maps to the one e4m3 twin
            L.set_switch("SVI_GEMM_KERNEL", forced)
            assert L.gemm_plan(300, 520, 576) == forced and w8_plan(300, 520, 576) == 260
            assert w8_plan(300, 520, 72) == 128          # K % 64 != 0: no 256-row tile for bf16 either
        L.set_switch("SVI_GEMM_KERNEL", 128)
        assert w8_plan(32760, 5120, 5120) == 128
        L.set_switch("SVI_GEMM_KERNEL", None)
        L.set_switch("SVI_GEMM_W8_256", 0)          # "0" is off, like unset
        for M, N, K, epi, skinny in SWEEP:
            assert w8_plan(M, N, K, epi, skinny) == today(L.gemm_plan(M, N, K, epi, skinny=skinny))
    finally:
        L.set_switch("SVI_GEMM_KERNEL", None)
        L.set_switch("SVI_GEMM_W8_256", None)
    for M, N, K, epi, skinny in SWEEP:
        assert w8_plan(M, N, K, epi, skinny) == today(L.gemm_plan(M, N, K, epi, skinny=skinny)), (M, N, K, epi, skinny)


def test_code_object_of_the_w8_256_kernel(tmp_path):
    """Two waves per SIMD beside 128 accumulator registers: no spilled register, no scratch, at most 256 VGPRs."""
    t = kernel_table(tmp_path)
    got = {k: v for k, v in t.items() if k.startswith("gemm_w8_nt_256e_kernel")}
    assert len(got) == 1, sorted(got)
    (v,) = got.values()
    assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, v
    assert v["vgpr_count"] <= 256, v
