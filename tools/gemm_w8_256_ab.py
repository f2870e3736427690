"""A/B of the 256-row GEMM that reads e4m3 weights (gemm_w8_nt_256e_kernel, SVI_GEMM_W8_256=1) on the hot shapes of a 14B block, interleaved in one process.

    python tools/gemm_w8_256_ab.py [rounds] >> profiles/fp8_resident_256_ab.txt
Per shape (q/k/v, attn-out, ffn1, ffn2 at dim 5120, ffn 13824, L = 32760 tokens): three arms on the same operands —
    bf16 260      svi_gemm_bf16_pair on the widened copy, the planner's own choice (asserted to be id 260)
    e4m3 128      svi_gemm_bf16_w8, switch unset: the 128^2 tile (resident mode's default route)
    e4m3 260      svi_gemm_bf16_w8 with SVI_GEMM_W8_256=1: the new kernel
bit-compared first (every element of C), then timed alternately: median and minimum over the rounds, three launches per sample."""
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "stable-video-infinity_amd"))
import torch  # noqa: E402

from svi_hip import _lib as L  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
dev = torch.device("cuda")
g = torch.Generator(device=dev).manual_seed(0)
Ltok, D, F = 32760, 5120, 13824
lib = L.lib()
st = L.current_stream()
SHAPES = {
    "qkv    [L,D]x[D,D]": (Ltok, D, D, L.EPI_BIAS),
    "attn_o gate+res": (Ltok, D, D, L.EPI_BIAS_GATE_RES),
    "ffn1   gelu": (Ltok, F, D, L.EPI_BIAS_GELU_TANH),
    "ffn2   gate+res": (Ltok, D, F, L.EPI_BIAS_GATE_RES),
}
ARMS = ("bf16 260", "e4m3 128", "e4m3 260")


def w8_plan(M, N, K, epi):
    k = ctypes.c_int32(-1)
    L.check(lib.svi_gemm_w8_plan(M, N, K, epi, 0, 256, ctypes.byref(k)), "svi_gemm_w8_plan")
    return k.value


for name, (M, N, K, epi) in SHAPES.items():
    x = torch.randn((M, K), generator=g, device=dev).to(torch.bfloat16)
    w8 = (torch.randn((N, K), generator=g, device=dev) * K ** -0.5).to(torch.float8_e4m3fn)
    wb = w8.to(torch.bfloat16)
    b = torch.randn(N, generator=g, device=dev).to(torch.bfloat16)
    gate = torch.randn(N, generator=g, device=dev)
    res = torch.randn((M, N), generator=g, device=dev).to(torch.bfloat16)
    outs = {a: torch.zeros((M, N), dtype=torch.bfloat16, device=dev) for a in ARMS}

    def run(arm):
        fn, w = (lib.svi_gemm_bf16_pair, wb) if arm == "bf16 260" else (lib.svi_gemm_bf16_w8, w8)
        L.check(fn(x.data_ptr(), K, w.data_ptr(), K, outs[arm].data_ptr(), N, M, N, K, b.data_ptr(), 0, epi,
                   gate.data_ptr() if epi == L.EPI_BIAS_GATE_RES else None, res.data_ptr() if epi == L.EPI_BIAS_GATE_RES else None, N,
                   None, None, 0, 0, 0, st), arm)

    def select(arm):
        L.set_switch("SVI_GEMM_W8_256", 1 if arm == "e4m3 260" else None)
        plan = L.gemm_plan(M, N, K, epi) if arm == "bf16 260" else w8_plan(M, N, K, epi)
        assert plan == int(arm.split()[1]), (name, arm, plan)

    for arm in ARMS:
        select(arm)
        run(arm)
    torch.cuda.synchronize()
    nbad = max(int((outs[ARMS[0]].view(torch.int16) != outs[a].view(torch.int16)).sum()) for a in ARMS[1:])
    times = {a: [] for a in ARMS}
    for _ in range(rounds):
        for arm in ARMS:
            select(arm)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(3):
                run(arm)
            e1.record()
            torch.cuda.synchronize()
            times[arm].append(e0.elapsed_time(e1) / 3)
    L.set_switch("SVI_GEMM_W8_256", None)
    fl = 2.0 * M * N * K
    msg = f"{name:20s} M={M} N={N} K={K}  mismatching={nbad}"
    for arm in ARMS:
        med, mn = statistics.median(times[arm]), min(times[arm])
        msg += f"  | {arm}: {med * 1e3:7.1f} us med {mn * 1e3:7.1f} min {fl / med / 1e9:6.0f} TFLOP/s"
    print(msg, flush=True)
