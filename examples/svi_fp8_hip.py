"""examples/test_svi_hip.py in the reference's FP8 storage mode (test_svi.py:337, load_models(torch_dtype=torch.float8_e4m3fn)): the DiT's parameters are cast
to float8_e4m3fn on the device as they are loaded (svi_hip.checkpoint.load_dit(torch_dtype=...), selected here through checkpoint.dit_storage), and the SVI
LoRA files are merged into the stored bytes — fp32 arithmetic, re-quantised, what the reference's loader does in that mode (svi_hip.lora.load_lora_ ->
svi_lora_merge_e4m3).  Everything else — the argument surface, the loading sequence, the encoders, the VAE, the resident clip loop, the outputs — is
test_svi_hip.py's own code, run as it is: that script is executed by the test suite (tests/test_gpu_stream.py, tests/test_reference_keys.py) and stays
untouched, so the FP8 mode is a script beside it that wraps its two model builders and calls its main().

--fp8_resident (or SVI_FP8_RESIDENT=1 in the environment): the blocks' Linear weights stay the stored e4m3 bytes — no bf16 copies; the GEMMs widen them on the way into the
matrix pipe (WanDiT.bind(fp8_resident=True)): the same video bit for bit, one byte per parameter resident.  The bound bytes are printed either way.
With SVI_GEMM_W8_256=1 beside it (opt-in) the large projections run on the 256-row tile that reads the stored bytes instead of the 128² tile: the same bits, faster at 14B sizes.

    python examples/svi_fp8_hip.py --synthetic --synthetic_model tiny-i2v --num_clips 3 --num_steps 4
    python examples/svi_fp8_hip.py --synthetic --synthetic_model tiny-i2v --num_clips 3 --num_steps 4 --fp8_resident
    python examples/svi_fp8_hip.py --dit_root weights/Wan2.1-I2V-14B-480P/ --extra_module_root weights/Stable-Video-Infinity/version-1.0/svi-shot.safetensors \\
        --ref_image_path data/cat.png --prompt_path data/cat_prompt.txt --num_clips 10
"""
from __future__ import annotations

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import test_svi_hip as base  # noqa: E402  (also puts the package and tests/ on sys.path)
import torch  # noqa: E402

_bf16_synthetic_models, _bf16_real_models = base.synthetic_models, base.real_models
_resident = None          # --fp8_resident: True; otherwise None = WanDiT.bind's default (SVI_FP8_RESIDENT, else False)


def synthetic_models(name: str, dev):
    """test_svi_hip.synthetic_models with the DiT's random-init weights stored as float8_e4m3fn."""
    from svi_hip.ops import f32_to_fp8_e4m3
    dit, vae, clip_encoder, embed = _bf16_synthetic_models(name, dev)
    dit.bind({k: f32_to_fp8_e4m3(v) for k, v in dit._params.items()}, fp8_resident=_resident)
    print(f"DiT weight bytes bound: {dit.weight_bytes()}")
    return dit, vae, clip_encoder, embed


def real_models(args, dev):
    """test_svi_hip.real_models as it stands — shards, LoRA files, VAE, encoders, tokenizer — with the DiT loaded into FP8 storage
    (checkpoint.dit_storage: its load_dit call stores every parameter as e4m3); load_lora_ then merges into the stored bytes."""
    from svi_hip import checkpoint
    with checkpoint.dit_storage(torch.float8_e4m3fn):
        models = _bf16_real_models(args, dev)
    assert models[0]._fp8_sources, "the DiT was not loaded into FP8 storage"
    if _resident and not models[0].weight_bytes()["e4m3"]:          # bound with bf16 copies by the builder: bind the stored tensors themselves, the copies are freed
        models[0].bind(dict(models[0]._fp8_sources), fp8_resident=True)
    print(f"DiT weight bytes bound: {models[0].weight_bytes()}")
    return models


def main(argv=None) -> dict:
    global _resident
    argv = list(sys.argv[1:] if argv is None else argv)
    _resident = True if "--fp8_resident" in argv else None          # this script's one flag of its own, taken out before test_svi_hip parses the rest
    argv = [a for a in argv if a != "--fp8_resident"]
    base.synthetic_models, base.real_models = synthetic_models, real_models          # main() builds its models through these two
    try:
        return base.main(argv)
    finally:
        base.synthetic_models, base.real_models = _bf16_synthetic_models, _bf16_real_models


if __name__ == "__main__":
    main()
