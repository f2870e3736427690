"""The case table of the encoder-kernel GPU tests (tests/encoder_kernel_cases.py) reaches what it claims — checked on the host: every
skinny case's seven projections plan onto the weight-streaming kernel (svi_gemm_plan == 0) and the comparison run onto a tiled one, the
launcher's rule restated here says which gemm_skinny_kernel<MB, NW, UN> each of them is and how many main / tail steps a wave walks, the
union covers every cell of SKINNY_CELLS, and every attention launch fits the LDS the kernel opts into."""
import pytest

import encoder_kernel_cases as ek
from svi_hip import _lib as L


def skinny_instance(M, K):
    """svi_launch_gemm's choice for a plan-0 GEMM, and gemm_skinny_kernel's two K loops: (MB, NW, UN, main steps, tail steps)."""
    assert 1 <= M <= 128
    mb = 1 if M <= 16 else 2 if M <= 32 else 4 if M <= 64 else 8
    nw = 8 if K % 256 == 0 else 4
    un = 4 if mb == 8 else 8
    assert K % (32 * nw) == 0, f"K = {K}: a wave's share {K}/{nw} is not a whole number of 32-steps (the kernel would drop or overrun K)"
    share = K // nw
    main = share // (32 * un)
    tail = (share - main * 32 * un) // 32
    assert main * 32 * un + tail * 32 == share
    return mb, nw, un, main, tail


def test_epilogue_codes_are_the_librarys():
    assert (ek.EPI_BIAS, ek.EPI_BIAS_GATE_RES) == (L.EPI_BIAS, L.EPI_BIAS_GATE_RES)


@pytest.mark.parametrize("name,M", ek.SKINNY_CASES)
def test_skinny_cases_take_the_skinny_kernel_and_their_comparison_a_tiled_one(name, M):
    cfg = ek.T5_CONFIGS[name]
    assert cfg["num_layers"] == 1 and cfg["vocab"] <= 512 and cfg["num_buckets"] == 32 and cfg["shared_pos"] is False
    assert 1 <= M <= 128 < ek.SKINNY_L
    shapes = ek.t5_gemm_shapes(cfg, M)
    assert len(shapes) == 7
    for proj, m, n, k, epi in shapes:
        assert L.gemm_plan(m, n, k, epi, skinny=True) == 0, (name, proj, m, n, k)
        skinny_instance(m, k)                                              # K / NW is a multiple of 32
    for proj, m, n, k, epi in ek.t5_gemm_shapes(cfg, ek.SKINNY_L):         # rows="all": M = L = 160 rows
        assert L.gemm_plan(m, n, k, epi, skinny=True) != 0, (name, proj, m, n, k)


def test_the_key_cases_run_tiled_gemms():
    """M > 128 in every key-axis case: those test the attention kernel alone."""
    cfg = ek.T5_CONFIGS["keys"]
    for case, Ln, valid, rows in ek.KEY_CASES + ek.KEY_BASELINE_CASES:
        assert 1 <= valid <= Ln <= ek.KEY_LIMIT and rows in ("all", "valid")
        for proj, m, n, k, epi in ek.t5_gemm_shapes(cfg, Ln if rows == "all" else valid):
            assert L.gemm_plan(m, n, k, epi, skinny=True) != 0, (case, proj)


def test_skinny_cases_cover_every_loop_of_every_instantiation():
    reached = {}
    for name, M in ek.SKINNY_CASES:
        for proj, m, n, k, epi in ek.t5_gemm_shapes(ek.T5_CONFIGS[name], M):
            mb, nw, un, main, tail = skinny_instance(m, k)
            assert un == (4 if mb == 8 else 8)
            loops = "main" if main and not tail else "main+tail" if main and tail else "tail"
            reached.setdefault((mb, nw, loops), []).append((name, M, proj, k, main, tail))
    missing = [cell for cell in ek.SKINNY_CELLS if cell not in reached]
    assert not missing, f"no case runs gemm_skinny_kernel (MB, NW, loops) = {missing}"
    assert len(ek.SKINNY_CELLS) == 12
    # the arithmetic the table's docstring states
    assert skinny_instance(16, 2304) == (1, 8, 8, 1, 1) and skinny_instance(128, 2304) == (8, 8, 4, 2, 1)
    assert skinny_instance(33, 2048) == (4, 8, 8, 1, 0) and skinny_instance(65, 2048) == (8, 8, 4, 2, 0)
    assert skinny_instance(17, 2560) == (2, 8, 8, 1, 2) and skinny_instance(100, 2560) == (8, 8, 4, 2, 2)
    assert skinny_instance(1, 1152) == (1, 4, 8, 1, 1) and skinny_instance(128, 1152) == (8, 4, 4, 2, 1)
    assert skinny_instance(64, 640) == (4, 4, 8, 0, 5) and skinny_instance(65, 640) == (8, 4, 4, 1, 1)
    assert skinny_instance(32, 1408) == (2, 4, 8, 1, 3) and skinny_instance(100, 1408) == (8, 4, 4, 2, 3)
    assert skinny_instance(40, 1024) == (4, 8, 8, 0, 4) and skinny_instance(128, 1024) == (8, 8, 4, 1, 0)
    # both sides of every MB boundary, per width
    for name in ("wide", "narrow"):
        assert sorted(M for c, M in ek.SKINNY_CASES if c == name) == [1, 16, 17, 32, 33, 64, 65, 100, 128]
    assert sorted(M for c, M in ek.SKINNY_CASES if c == "d32") == [16, 40, 128]


def test_attention_cases_cover_the_head_sizes_and_fit_the_lds():
    opted = 160 * 1024 - 256                                  # launch_enc_attention's svi_ensure_lds
    launches = ek.attention_launches()
    for name, D, Lk in launches:
        assert D in (32, 64, 80, 128) and 1 <= Lk <= ek.KEY_LIMIT, (name, D, Lk)
        assert ek.attention_lds_bytes(D, Lk) <= opted, (name, D, Lk)
    assert {D for name, D, Lk in launches if not name.startswith("clip_")} >= {32, 80, 128}          # bf16 (64: tests/test_gpu_encoders.py)
    assert {D for name, D, Lk in launches if name.startswith("clip_")} == {32, 64, 128}              # fp32 (80: tests/test_gpu_encoders.py)
    limit = [(D, Lk) for name, D, Lk in launches if name == "limit2048"]
    assert limit == [(128, 2048)] and ek.attention_lds_bytes(*limit[0]) >= 128 * 1024
    assert ("odd1025", 128, 1025) in launches and 1025 % 256 == 1 and 1025 % 64 == 1
    assert ("full512", 128, 512) in launches
