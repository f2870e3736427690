"""-m gpu: FP8-resident weights on the 256-row route (SVI_GEMM_W8_256 = 1; gemm_w8_nt_256e_kernel, csrc/svi_gemm.hip).

The tiny synthetic models of tests/test_gpu_fp8_resident.py, stored as e4m3.  SVI_GEMM_KERNEL = 260 sends every bf16 projection of the non-resident model
to the two-phase 256^2 tile; with SVI_GEMM_W8_256 = 1 beside it the resident model's projections with W stored as e4m3 take the same id on the kernel that
reads the stored bytes (asserted on both planners before the forward).  That kernel gives the bits of its bf16 twin (tests/test_gpu_gemm_w8_256.py), and
the transposed value projection — the A-operand form, which stays on the 128^2 tile — gives them as every tile kind does: torch.equal."""
import ctypes

import pytest
import torch

from test_gpu_fp8_resident import build, listed, stored_e4m3
from test_oracle_dit import CASES

pytestmark = pytest.mark.gpu

MIXED = "blocks.0.self_attn.k.weight"          # bound as bf16 in the "mixed" case while its partner q stays e4m3: svi_dit.hip splits the q | k launch in two


def assert_plans_to_260(L, c, grid):
    """The block's [L, D] x {D, 2D (q | k), F} and [L, F] x D projections, for one sample: the bf16 planner and the e4m3 planner both say 260."""
    D, F = c["dim"], c["ffn_dim"]
    tokens = grid[0] * grid[1] * grid[2]
    for M, N, K in ((tokens, D, D), (tokens, 2 * D, D), (tokens, F, D), (tokens, D, F)):
        k = ctypes.c_int32(-1)
        assert L.lib().svi_gemm_w8_plan(M, N, K, 0, 0, 256, ctypes.byref(k)) == 0
        assert L.gemm_plan(M, N, K) == 260 and k.value == 260, (M, N, K, L.gemm_plan(M, N, K), k.value)


@pytest.mark.parametrize("name,mixed", [(n, False) for n in CASES] + [("tiny_t2v", True)])
def test_forward_bits_on_the_256_row_route(name, mixed):
    from svi_hip import _lib as L
    c, sd, x, ctx, ts, kw, grid = stored_e4m3(name)
    if mixed:
        sd[MIXED] = sd[MIXED].to(torch.bfloat16)          # the same values; from_state_dict keeps a bf16 tensor bf16
    try:
        L.set_switch("SVI_GEMM_KERNEL", 260)
        plain = build(c, sd, False)
        assert plain.weight_bytes()["e4m3"] == 0
        want = plain.forward(x, ts, ctx, **kw).clone()
        del plain
        L.set_switch("SVI_GEMM_W8_256", 1)
        assert_plans_to_260(L, c, grid)
        m = build(c, sd, True)
        names = listed(m)
        resident = [k for k in names if m._params[k].dtype == torch.float8_e4m3fn]
        assert len(resident) == len(names) - (1 if mixed else 0) and (MIXED in resident) != mixed
        assert "blocks.0.self_attn.q.weight" in resident
        got = m.forward(x, ts, ctx, **kw)
        assert torch.isfinite(got.float()).all()
        assert torch.equal(got, want)
    finally:
        L.set_switch("SVI_GEMM_W8_256", None)
        L.set_switch("SVI_GEMM_KERNEL", None)
