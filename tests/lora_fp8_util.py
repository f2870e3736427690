"""Shared by tests/test_lora_fp8_host.py and tests/test_gpu_lora_fp8.py: the cases of tests/golden/lora_fp8.npz (the reference's LoRA merge
into float8_e4m3fn parameters, tests/gen_golden_lora_fp8.py) and the acceptance band of a merged code.

The band.  The merge is e4m3(fl(W + fl(alpha * fl(sum_k up_k down_k)))) with fp32 roundings fl; only the order of the r-term sum is free.  With s the
exact value (fp64) and  d = (r + 2) * 2^-24 * (|W| + |alpha| * |up| . |down|)  — r - 1 additions and the product roundings inside the sum, one
rounding for the scaling, one for the addition, each at most 2^-24 relative of a partial result that |W| + |alpha| |up| . |down| bounds — every
admissible fp32 result lies in [s - d, s + d], so every admissible code is cast(s - d) or cast(s + d) (the cast is monotone and d is far below an e4m3
step).  Where the two agree the code is determined and must be the reference's.
"""
import os

import numpy as np
import torch

from conftest import GOLDEN

CASE_NAMES = ("bf16_r32", "bf16_r128", "f32_r8", "sequence")
AMBIGUOUS_CAP = 0.01


def load_cases():
    """name -> dict(before uint8 [out, in], after uint8, files [(up, down, alpha)] with up / down torch tensors in their stored dtype)."""
    z = np.load(os.path.join(GOLDEN, "lora_fp8.npz"))
    cases = {}
    for name in CASE_NAMES:
        files = []
        for i in range(int(z[f"{name}.files"])):
            up, down = z[f"{name}.{i}.up"], z[f"{name}.{i}.down"]
            if up.dtype == np.uint16:
                up, down = torch.from_numpy(up.copy()).view(torch.bfloat16), torch.from_numpy(down.copy()).view(torch.bfloat16)
            else:
                up, down = torch.from_numpy(up.copy()), torch.from_numpy(down.copy())
            files.append((up, down, float(z[f"{name}.{i}.alpha"])))
        cases[name] = dict(before=z[f"{name}.before"].copy(), after=z[f"{name}.after"].copy(), files=files)
    return cases


def codes_to_f32(codes: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(codes)).view(torch.float8_e4m3fn).float()


def cast_codes(x: torch.Tensor) -> np.ndarray:
    """torch's CPU cast of an fp32 / fp64 tensor to e4m3fn, as uint8 codes (fp64 goes through fp32 first, which keeps the order)."""
    return x.to(torch.float32).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def torch_merge(before: np.ndarray, up: torch.Tensor, down: torch.Tensor, alpha: float) -> np.ndarray:
    """Our reading of GeneralLoRAFromPeft.load on fp8 parameters, on the CPU."""
    return cast_codes(codes_to_f32(before) + alpha * torch.mm(up.float(), down.float()))


def band(before: np.ndarray, up: torch.Tensor, down: torch.Tensor, alpha: float):
    """(codes of cast(s - d), codes of cast(s + d)) for one merge step; see the module docstring."""
    a = float(np.float32(alpha))                                  # the scaling runs in fp32: alpha enters as an fp32 number
    w, u, v = codes_to_f32(before).double(), up.double(), down.double()
    s = w + a * (u @ v)
    d = (up.shape[1] + 2) * 2.0 ** -24 * (w.abs() + abs(a) * (u.abs() @ v.abs()))
    return cast_codes(s - d), cast_codes(s + d)


def check_step(got: np.ndarray, before: np.ndarray, up, down, alpha, want: np.ndarray, label: str):
    """The criterion of the merge test for one step; returns the ambiguous share."""
    lo, hi = band(before, up, down, alpha)
    ambiguous = lo != hi
    share = float(ambiguous.mean())
    outside = int(((got != lo) & (got != hi)).sum())
    wrong = int(((got != want) & ~ambiguous).sum())
    print(f"{label}: ambiguous share {share:.4%}, codes outside the band {outside}, determined codes unlike the reference {wrong}, "
          f"codes unlike the reference in all {int((got != want).sum())} of {got.size}")
    assert share <= AMBIGUOUS_CAP, (label, share)
    assert outside == 0, (label, outside)
    assert wrong == 0, (label, wrong)
    return share
