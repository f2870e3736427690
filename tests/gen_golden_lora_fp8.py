"""Generate tests/golden/lora_fp8.npz: the REFERENCE's LoRA merge into float8_e4m3fn parameters.

GeneralLoRAFromPeft.load (diffsynth/models/lora.py:231-267) is compiled out of the reference's source file (gen_golden._reference_toplevel:
executed, not copied) and run on a tiny module whose parameters are float8_e4m3fn, which makes its computation dtype fp32.  Per case the
fixture keeps the e4m3 codes before, every LoRA file's up / down / alpha in application order, and the codes after.

    python tests/gen_golden_lora_fp8.py

bf16 operands are stored as their 16-bit patterns (uint16), fp32 operands as fp32.  Data: W ~ 0.05 N(0,1) quantised to e4m3, operands ~ 0.1 N(0,1).
"""
from __future__ import annotations

import io
import contextlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import synth  # noqa: E402
from gen_golden import OUT, _reference_toplevel  # noqa: E402

# name -> (out_f, in_f, seed, [(rank, alpha, operand dtype), ...] applied in this order)
CASES = {
    "bf16_r32": (200, 264, 4100, [(32, 2.0, "bf16")]),
    "bf16_r128": (256, 256, 4200, [(128, 1.0, "bf16")]),
    "f32_r8": (72, 136, 4300, [(8, 0.7, "f32")]),
    "sequence": (200, 264, 4400, [(16, 1.0, "bf16"), (8, 0.5, "f32")]),
}


class _Holder(torch.nn.Module):
    """One parameter named `w.weight`, stored as float8_e4m3fn."""

    def __init__(self, w8: torch.Tensor):
        super().__init__()
        self.w = torch.nn.Module()
        self.w.weight = torch.nn.Parameter(w8, requires_grad=False)


def reference_loader():
    ns = {"torch": torch}
    for name in ("SDUNet", "SDXLUNet", "SD3DiT", "HunyuanDiT", "FluxDiT", "CogDiT", "WanModel"):      # only listed by __init__, never used by load
        ns[name] = type(name, (), {})
    return _reference_toplevel("diffsynth/models/lora.py", "GeneralLoRAFromPeft", ns)()


def operands(seed: int, out_f: int, in_f: int, r: int, dtype: str):
    up, down = 0.1 * synth.randn(seed, out_f, r), 0.1 * synth.randn(seed + 1, r, in_f)
    up, down = torch.from_numpy(up), torch.from_numpy(down)
    if dtype == "bf16":
        up, down = up.to(torch.bfloat16), down.to(torch.bfloat16)
    return up, down


def main():
    loader = reference_loader()
    out = {}
    for name, (out_f, in_f, seed, files) in CASES.items():
        w8 = torch.from_numpy(0.05 * synth.randn(seed, out_f, in_f)).to(torch.float8_e4m3fn)
        m = _Holder(w8.clone())
        out[f"{name}.before"] = w8.view(torch.uint8).numpy().copy()
        out[f"{name}.files"] = np.int64(len(files))
        for i, (r, alpha, dtype) in enumerate(files):
            up, down = operands(seed + 10 * (i + 1), out_f, in_f, r, dtype)
            with contextlib.redirect_stdout(io.StringIO()):
                loader.load(m, {"w.lora_B.weight": up, "w.lora_A.weight": down}, alpha=alpha)
            assert m.w.weight.dtype == torch.float8_e4m3fn
            out[f"{name}.{i}.up"] = up.view(torch.uint16).numpy() if dtype == "bf16" else up.numpy()
            out[f"{name}.{i}.down"] = down.view(torch.uint16).numpy() if dtype == "bf16" else down.numpy()
            out[f"{name}.{i}.alpha"] = np.float64(alpha)
        out[f"{name}.after"] = m.w.weight.data.view(torch.uint8).numpy().copy()
        changed = float((out[f"{name}.after"] != out[f"{name}.before"]).mean())
        print(f"{name}: [{out_f}, {in_f}] {files}: {changed:.1%} of the codes changed")
    path = os.path.join(OUT, "lora_fp8.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
