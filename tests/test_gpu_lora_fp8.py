"""-m gpu: LoRA merge into FP8-stored weights (svi_lora_merge_e4m3, svi_f32_to_fp8_e4m3; csrc/svi_lora.hip).

  cast     svi_f32_to_fp8_e4m3 is torch's `.to(torch.float8_e4m3fn)` bit for bit (a NaN may carry either sign): every code, every rounding tie and its
           fp32 neighbours, the subnormal floor, the no-saturation rule above 464, random values; from fp32 and from bf16
  merge    every case of tests/golden/lora_fp8.npz (the reference's own loader on fp8 parameters): each code inside the fp32 accumulation-order band
           of lora_fp8_util, equal to the reference's wherever the band determines it; in place, version counter bumped
  edges    a weight carved out of a larger buffer: the bytes around it stay; bad rank / mismatched pair -> ValueError
  model    load_lora_ on a WanDiT in FP8 storage mode == a fresh model built from the merged codes (bf16 copies re-cast, context cache dropped,
           MX-fp8 MLP pointers re-bound)
  loader   checkpoint.load_dit(torch_dtype=torch.float8_e4m3fn) stores every parameter as torch's cast of it
  example  examples/svi_fp8_hip.py builds its DiT in FP8 storage and runs the clip loop on it
"""
import numpy as np
import pytest
import torch

import lora_fp8_util as U
import synth
from gpu_util import dev
from test_oracle_dit import CASES, inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return U.load_cases()


# ---------------------------------------------------------------------------------------------------------------- the cast
def cast_table() -> torch.Tensor:
    codes = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float()
    finite = torch.sort(codes[~torch.isnan(codes) & (codes >= 0)].unique()).values           # 0, 2^-9, ..., 448
    mid = ((finite[:-1].double() + finite[1:].double()) / 2).float()                          # exact in fp32: the ties
    inf = torch.tensor(float("inf"))
    mids = torch.cat([torch.nextafter(mid, -inf), mid, torch.nextafter(mid, inf)])
    tiny = torch.tensor(2.0 ** -10)
    special = torch.tensor([448.0, 463.99, 464.0, 464.01, 480.0, 1e9, float("inf"), float("-inf"), float("nan"), 0.0, -0.0, 1e-30])
    special = torch.cat([special, torch.stack([torch.nextafter(tiny, -inf), tiny, torch.nextafter(tiny, inf)])])
    rs = np.random.RandomState(77)
    rand = torch.from_numpy((rs.standard_normal(4096) * np.exp2(rs.uniform(-12, 9.5, 4096))).astype(np.float32))
    t = torch.cat([codes, mids, -mids, special, -special, rand])
    return t


def same_codes(got: np.ndarray, want: np.ndarray) -> np.ndarray:
    """Elementwise: equal, or both the NaN code (either sign)."""
    return (got == want) | (((got & 0x7f) == 0x7f) & ((want & 0x7f) == 0x7f))


@pytest.mark.parametrize("src", [torch.float32, torch.bfloat16])
def test_cast_is_torchs_cast(src):
    from svi_hip.ops import f32_to_fp8_e4m3
    x = cast_table().to(src)
    want = x.to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    for off in (0, 3):                                             # 3: an unaligned view, the element-by-element path
        xs = x.cuda()[off:]
        got8 = f32_to_fp8_e4m3(xs)
        assert got8.dtype == torch.float8_e4m3fn and got8.shape == xs.shape
        got = got8.view(torch.uint8).cpu().numpy()
        ok = same_codes(got, want[off:])
        bad = np.flatnonzero(~ok)
        print(f"cast from {src}, offset {off}: {x.numel() - off} values, {bad.size} differ")
        assert bad.size == 0, [(float(x[off + i]), hex(got[i]), hex(want[off + i])) for i in bad[:8]]
    xf = x.float().numpy()
    assert (want[np.abs(xf) > 464] & 0x7f == 0x7f).all() and (want[xf == 464] == 0x7e).all() and (want[xf == 2.0 ** -10] == 0).all()      # the table reaches the rules it names


# ---------------------------------------------------------------------------------------------------------------- the merge
def merged(before: np.ndarray, up, down, alpha):
    from svi_hip import lora
    w = torch.from_numpy(before.copy()).cuda().view(torch.float8_e4m3fn)
    ptr, ver = w.data_ptr(), w._version
    out = lora.merge_lora_(w, up, down, alpha)
    assert out is w and w.data_ptr() == ptr and w._version > ver and w.dtype == torch.float8_e4m3fn
    return w.view(torch.uint8).cpu().numpy()


@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_merge_is_the_references_merge(cases, name):
    c = cases[name]
    w, ref = c["before"], c["before"]
    for i, (up, down, alpha) in enumerate(c["files"]):
        nxt_ref = U.torch_merge(ref, up, down, alpha)              # the reference's codes after this file (test_lora_fp8_host pins the reading)
        if i == len(c["files"]) - 1:
            assert np.array_equal(nxt_ref, c["after"])
            nxt_ref = c["after"]
        # later files start from OUR codes of the earlier ones: where those equal the reference's, so must the result (the merge is elementwise in W)
        want = np.where(w == ref, nxt_ref, U.torch_merge(w, up, down, alpha))
        got = merged(w, up, down, alpha)
        U.check_step(got, w, up, down, alpha, want, f"{name}[{i}] kernel")
        w, ref = got, nxt_ref


def test_fp16_operands_keep_their_precision():
    """fp16 operands (not in the fixture) are widened exactly like the reference's `.to(float32)`: same band, against torch's CPU merge."""
    before = torch.from_numpy(0.05 * synth.randn(4500, 72, 136)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    up, down = torch.from_numpy(0.1 * synth.randn(4501, 72, 24)).half(), torch.from_numpy(0.1 * synth.randn(4502, 24, 136)).half()
    assert not torch.equal(up.float(), up.to(torch.bfloat16).float())
    got = merged(before, up, down, 0.7)
    U.check_step(got, before, up, down, 0.7, U.torch_merge(before, up, down, 0.7), "fp16 operands")


# ---------------------------------------------------------------------------------------------------------------- edges
def test_bytes_around_the_weight_stay(cases):
    from svi_hip import lora
    c = cases["f32_r8"]
    up, down, alpha = c["files"][0]
    out_f, in_f = c["before"].shape
    n, lead = out_f * in_f, 1000                                  # 1000: 8-byte aligned, not 16 — the 8-byte access path (in_f = 136 is no multiple of 16 either)
    buf = torch.full((lead + n + 4096,), 0x55, dtype=torch.uint8, device="cuda")
    buf[lead:lead + n] = torch.from_numpy(c["before"].reshape(-1)).cuda()
    w = buf[lead:lead + n].view(torch.float8_e4m3fn).view(out_f, in_f)
    lora.merge_lora_(w, up, down, alpha)
    host = buf.cpu().numpy()
    assert (host[:lead] == 0x55).all() and (host[lead + n:] == 0x55).all()
    U.check_step(host[lead:lead + n].reshape(out_f, in_f), c["before"], up, down, alpha, c["after"], "carved")


def test_bad_pairs_are_refused(cases):
    from svi_hip import lora
    w = torch.zeros(72, 136, device="cuda").to(torch.float8_e4m3fn)
    with pytest.raises(ValueError, match="multiples of 8"):
        lora.merge_lora_(w, torch.ones(72, 12), torch.ones(12, 136), 1.0)
    with pytest.raises(ValueError, match="does not match"):
        lora.merge_lora_(w, torch.ones(64, 8), torch.ones(8, 136), 1.0)
    with pytest.raises(ValueError, match="does not match"):
        lora.merge_lora_(w, torch.ones(72, 8), torch.ones(16, 136), 1.0)
    with pytest.raises(ValueError, match=r"\(72, 8, 1, 1\) x \(4, 136, 1, 1\)"):        # the message shows the shapes the caller passed
        lora.merge_lora_(w, torch.ones(72, 8, 1, 1), torch.ones(4, 136, 1, 1), 1.0)
    assert not w.view(torch.uint8).any()


# ---------------------------------------------------------------------------------------------------------------- through the model
TARGETS = ("blocks.0.cross_attn.k", "blocks.1.ffn.0")          # a prompt-side projection (cached K) and an MLP matrix (MX-fp8 pointer)


def tiny_fp8_model():
    import svi_hip
    c, grid, nt, nv, ts, seed = CASES["tiny_t2v"]
    sd = {k: torch.from_numpy(v).to(torch.float8_e4m3fn) for k, v in synth.dit_state_dict(seed, **c).items()}
    m = svi_hip.WanDiT.from_state_dict(sd, eps=1e-6, num_heads=synth.num_heads_of(c), **c)
    x, ctx, _ = inputs(c, grid, nt, nv, seed)
    return m, c, dev(x), dev(ctx), torch.tensor([ts])


@pytest.mark.parametrize("fp8_mlp", [False, True])
def test_load_lora_through_the_model(fp8_mlp):
    import svi_hip
    from svi_hip import lora
    m, c, x, ctx, ts = tiny_fp8_model()
    if fp8_mlp:
        m.ffn_fp8_mfma(True)
    m.context_cache(True)                                          # the cached cross-attention K / V were projected with the old weights
    before = m.forward(x, ts, ctx).clone()
    file = {}
    for i, t in enumerate(TARGETS):
        out_f, in_f = m._fp8_sources[t + ".weight"].shape
        file[f"diffusion_model.{t}.lora_B.default.weight"] = torch.from_numpy(0.1 * synth.randn(4600 + 2 * i, out_f, 8)).to(torch.bfloat16)
        file[f"diffusion_model.{t}.lora_A.default.weight"] = torch.from_numpy(0.1 * synth.randn(4601 + 2 * i, 8, in_f)).to(torch.bfloat16)
    ptrs = {t: m._fp8_sources[t + ".weight"].data_ptr() for t in TARGETS}
    assert lora.load_lora_(m, file, alpha=0.7) == 2
    assert all(m._fp8_sources[t + ".weight"].data_ptr() == p for t, p in ptrs.items()) and not m.weights_changed()
    after = m.forward(x, ts, ctx).clone()
    assert not torch.equal(after, before)
    fresh = svi_hip.WanDiT.from_state_dict({k: v.clone() for k, v in m._fp8_sources.items()}, eps=1e-6, num_heads=synth.num_heads_of(c), **c)
    assert len(fresh._fp8_sources) == len(m._fp8_sources)
    if fp8_mlp:
        fresh.ffn_fp8_mfma(True)
    assert torch.equal(fresh.forward(x, ts, ctx), after)


def test_merge_state_dict_on_a_mixed_dict(cases):
    """bf16 and fp8 tensors side by side: each merged in its own dtype, the bf16 one exactly as before."""
    from svi_hip import lora
    c = cases["bf16_r32"]
    up, down, alpha = c["files"][0]
    w8 = torch.from_numpy(c["before"].copy()).cuda().view(torch.float8_e4m3fn)
    w16 = U.codes_to_f32(c["before"]).to(torch.bfloat16).cuda()
    alone = lora.merge_lora_(w16.clone(), up, down, alpha)
    sd = {"a.weight": w8, "b.weight": w16}
    assert lora.merge_state_dict_(sd, {"a.weight": (up, down), "b.weight": (up, down)}, alpha) == 2
    assert torch.equal(sd["b.weight"], alone) and sd["b.weight"].dtype == torch.bfloat16
    U.check_step(w8.view(torch.uint8).cpu().numpy(), c["before"], up, down, alpha, c["after"], "mixed dict")


# ---------------------------------------------------------------------------------------------------------------- the loader
def test_load_dit_stores_every_parameter_as_e4m3(tmp_path):
    from safetensors.torch import save_file
    from svi_hip import checkpoint
    c, grid, nt, nv, ts, seed = CASES["tiny_t2v"]
    sd = {k: torch.from_numpy(v).to(torch.bfloat16) for k, v in synth.dit_state_dict(seed, **c).items()}
    path = str(tmp_path / "dit.safetensors")
    save_file(sd, path)
    m = checkpoint.load_dit(path, torch_dtype=torch.float8_e4m3fn)
    assert set(m._fp8_sources) == set(sd)
    for k, v in sd.items():
        got = m._fp8_sources[k]
        assert got.dtype == torch.float8_e4m3fn and got.shape == v.shape, k
        assert torch.equal(got.view(torch.uint8).cpu(), v.to(torch.float8_e4m3fn).view(torch.uint8)), k
    plain = checkpoint.load_dit(path)
    assert not plain._fp8_sources                                  # None keeps today's behaviour
    with checkpoint.dit_storage(torch.float8_e4m3fn):              # the same selection from outside the call (examples/svi_fp8_hip.py)
        inside = checkpoint.load_dit(path)
    assert set(inside._fp8_sources) == set(sd) and not checkpoint.load_dit(path)._fp8_sources
    assert all(torch.equal(inside._fp8_sources[k].view(torch.uint8), m._fp8_sources[k].view(torch.uint8)) for k in sd)
    x, ctx, _ = inputs(c, grid, nt, nv, seed)
    assert torch.isfinite(m.forward(dev(x), torch.tensor([ts]), dev(ctx)).float()).all()


# ---------------------------------------------------------------------------------------------------------------- the example
def test_fp8_example_runs_on_fp8_stored_weights(tmp_path):
    """examples/svi_fp8_hip.py (in process, toy sizes): the synthetic DiT it builds is FP8-stored throughout, and the rolling window runs on it."""
    import importlib.util
    import os
    import sys
    from conftest import ROOT
    ex = os.path.join(ROOT, "examples")
    sys.path.insert(0, ex)
    try:
        spec = importlib.util.spec_from_file_location("svi_fp8_hip_example", os.path.join(ex, "svi_fp8_hip.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        dit = mod.synthetic_models("tiny-i2v", torch.device("cuda", 0))[0]
        assert dit._fp8_sources and set(dit._fp8_sources) == set(dit._params)
        out = mod.main(["--synthetic", "--synthetic_model", "tiny-i2v", "--num_clips", "2", "--num_steps", "2", "--height", "64", "--width", "96",
                        "--max_frames", "9", "--output", str(tmp_path)])
    finally:
        sys.path.remove(ex)
    rec = out["test_svi_hip"][0]
    assert rec["clips"] == 2 and rec["frames"] == 17
    assert mod.base.synthetic_models is not mod.synthetic_models            # the stand-ins were handed back
