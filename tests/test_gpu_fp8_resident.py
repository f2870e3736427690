"""-m gpu: FP8-resident weights (WanDiT.bind(fp8_resident=True)) on the tiny synthetic models stored as e4m3.

The e4m3 GEMM forms are bit-identical to the bf16 kernels on the widened copy (tests/test_gpu_gemm_w8.py) when both run on the same kernel id, so a
resident model must give the bits of the non-resident one: torch.equal throughout.  Every launch of these models plans to the 128^2 tile in both modes
(asserted here on the planners), which is what lets the comparison lean on that."""
import ctypes

import pytest
import torch

import synth
from gpu_util import dev
from test_oracle_dit import CASES, inputs

pytestmark = pytest.mark.gpu


def stored_e4m3(name):
    c, grid, nt, nv, ts, seed = CASES[name]
    sd = {k: torch.from_numpy(v).to(torch.float8_e4m3fn) for k, v in synth.dit_state_dict(seed, **c).items()}
    x, ctx, kw = inputs(c, grid, nt, nv, seed)
    return c, sd, dev(x), dev(ctx), torch.tensor([ts]), {k: dev(v) for k, v in kw.items()}, grid


def build(c, sd, resident):
    import svi_hip
    return svi_hip.WanDiT.from_state_dict({k: v.clone() for k, v in sd.items()}, eps=1e-6, num_heads=synth.num_heads_of(c), fp8_resident=resident, **c)


def listed(m):
    from svi_hip.dit import _FP8_RESIDENT_KEY
    return [k for k in m._params if _FP8_RESIDENT_KEY.match(k)]


def assert_plans_to_128(c, grid, ctx_tokens, extra_rows=()):
    """Every projection of a block, for one sample and for a stacked pair, as the DiT shapes it: [L, D] x {D, 2D (q | k), F}, the transposed value
    projections [D, D] x [L | Lc | 257, D], the prompt-side K [Lc | 257, D], the audio projections (K = 768): the bf16 planner and the e4m3 planner both
    say 128.  extra_rows: further row counts (a shard's rows, the audio tokens)."""
    from svi_hip import _lib as L
    D, F = c["dim"], c["ffn_dim"]
    tokens = grid[0] * grid[1] * grid[2]
    shapes = []
    for rows in (tokens, 2 * tokens, ctx_tokens, 257) + tuple(extra_rows):
        shapes += [(rows, D, D), (rows, 2 * D, D), (rows, F, D), (rows, D, F), (D, rows, D), (rows, D, 768), (D, rows, 768)]
    for M, N, K in shapes:
        k = ctypes.c_int32(-1)
        assert L.lib().svi_gemm_w8_plan(M, N, K, 0, 0, 256, ctypes.byref(k)) == 0
        assert L.gemm_plan(M, N, K) == 128 and k.value == 128, (M, N, K, L.gemm_plan(M, N, K), k.value)


@pytest.mark.parametrize("name", list(CASES))
def test_forward_bits_bytes_and_memory(name):
    c, sd, x, ctx, ts, kw, grid = stored_e4m3(name)
    assert_plans_to_128(c, grid, ctx.shape[1])
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    plain = build(c, sd, False)
    torch.cuda.synchronize()
    used_plain = torch.cuda.memory_allocated() - base
    want = plain.forward(x, ts, ctx, **kw).clone()
    assert plain.weight_bytes()["e4m3"] == 0
    del plain
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    m = build(c, sd, True)
    torch.cuda.synchronize()
    used = torch.cuda.memory_allocated() - base
    names = listed(m)
    n8 = sum(m._params[k].numel() for k in names)
    per_block = 10 + (2 if c["has_image_input"] else 0)
    assert len(names) == per_block * c["num_layers"] and n8 > 0
    for k in names:          # the stored tensor itself is what is bound: no bf16 tensor exists for it
        assert m._params[k] is m._fp8_sources[k] and m._params[k].dtype == torch.float8_e4m3fn
    assert all(t.dtype == torch.bfloat16 for k, t in m._params.items() if k not in names)
    wb = m.weight_bytes()
    assert wb["e4m3"] == n8 and wb["bf16"] == 2 * sum(t.numel() for k, t in m._params.items() if k not in names)
    assert used <= used_plain - 2 * n8, (used, used_plain, n8)
    got = m.forward(x, ts, ctx, **kw)
    assert torch.equal(got, want)
    assert not m.weights_changed()
    m._params[names[0]].view(torch.uint8)[0, 0] ^= 1          # an in-place write to a resident weight is seen
    assert m.weights_changed()


def test_rebind_casts_nothing_for_resident_weights():
    c, sd, x, ctx, ts, kw, _ = stored_e4m3("tiny_t2v")
    m = build(c, sd, True)
    before = {k: m._params[k].data_ptr() for k in listed(m)}
    want, wb = m.forward(x, ts, ctx).clone(), m.weight_bytes()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    m.rebind()
    torch.cuda.synchronize()
    assert {k: m._params[k].data_ptr() for k in listed(m)} == before and m.weight_bytes() == wb
    assert all(m._params[k] is m._fp8_sources[k] for k in before)
    assert torch.cuda.memory_allocated() - base <= 0
    assert torch.equal(m.forward(x, ts, ctx), want)


def test_load_lora_on_a_resident_model():
    from svi_hip import lora
    c, sd, x, ctx, ts, kw, _ = stored_e4m3("tiny_t2v")
    targets = ("blocks.0.cross_attn.k", "blocks.1.ffn.0", "blocks.0.self_attn.v")
    file = {}
    for i, t in enumerate(targets):
        out_f, in_f = sd[t + ".weight"].shape
        file[f"diffusion_model.{t}.lora_B.default.weight"] = torch.from_numpy(0.1 * synth.randn(4700 + 2 * i, out_f, 8)).to(torch.bfloat16)
        file[f"diffusion_model.{t}.lora_A.default.weight"] = torch.from_numpy(0.1 * synth.randn(4701 + 2 * i, 8, in_f)).to(torch.bfloat16)
    outs = []
    for resident in (True, False):
        m = build(c, sd, resident)
        m.context_cache(True)
        before, wb = m.forward(x, ts, ctx).clone(), m.weight_bytes()
        assert lora.load_lora_(m, file, alpha=0.7) == len(targets)
        assert m.weight_bytes() == wb
        after = m.forward(x, ts, ctx).clone()
        assert not torch.equal(after, before)
        outs.append(after)
    assert torch.equal(outs[0], outs[1])


def test_ffn_fp8_mfma_on_a_resident_model():
    c, sd, x, ctx, ts, kw, _ = stored_e4m3("tiny_t2v")
    outs = []
    for resident in (True, False):
        m = build(c, sd, resident)
        m.ffn_fp8_mfma(True)
        outs.append(m.forward(x, ts, ctx).clone())
    assert torch.equal(outs[0], outs[1])


def test_resident_is_a_no_op_for_bf16_parameters():
    import svi_hip
    c, sd, x, ctx, ts, kw, _ = stored_e4m3("tiny_t2v")
    sd16 = {k: v.to(torch.bfloat16) for k, v in sd.items()}
    outs = []
    for resident in (True, False):
        m = svi_hip.WanDiT.from_state_dict(sd16, eps=1e-6, num_heads=synth.num_heads_of(c), fp8_resident=resident, **c)
        assert m.weight_bytes()["e4m3"] == 0 and not m._fp8_sources
        outs.append(m.forward(x, ts, ctx).clone())
    assert torch.equal(outs[0], outs[1])


def test_environment_default(monkeypatch):
    c, sd, x, ctx, ts, kw, _ = stored_e4m3("tiny_t2v")
    monkeypatch.setenv("SVI_FP8_RESIDENT", "1")
    assert build(c, sd, None).weight_bytes()["e4m3"] > 0
    assert build(c, sd, False).weight_bytes()["e4m3"] == 0
    monkeypatch.delenv("SVI_FP8_RESIDENT")
    assert build(c, sd, None).weight_bytes()["e4m3"] == 0


# ---- the step loops, the talk step and the shards: every path through the one projection helper --------------------------------------------------------
CLIP_GRID, NT, NV, TEA_THRESH = (3, 4, 6), 20, 13, -2.0e4          # tests/test_gpu_teacache_graph.py's clip: at this threshold the 8-step clip computes and skips


def clip_pair():
    """The tiny T2V model stored as e4m3, bound resident and not (context cache on), and one clip's latents and prompts."""
    c, seed = synth.TINY_DIT, 100
    sd = {k: torch.from_numpy(v).to(torch.float8_e4m3fn) for k, v in synth.dit_state_dict(seed, **c).items()}
    f, h, w = CLIP_GRID
    lat = dev(synth.randn(seed + 1, 1, 16, f, 2 * h, 2 * w))
    cp = dev(synth.text_context(seed + 2, NT, c["text_dim"], NV))
    cn = dev(synth.text_context(seed + 3, NT, c["text_dim"], NV - 4))
    assert_plans_to_128(c, CLIP_GRID, NT)
    models = []
    for resident in (True, False):
        m = build(c, sd, resident)
        m.context_cache(True)
        models.append(m)
    assert models[0].weight_bytes()["e4m3"] > 0 and models[1].weight_bytes()["e4m3"] == 0
    return models, lat, cp, cn


def test_graphed_denoise_clip():
    """Three steps of the graphed loop: the stacked CFG pair on cached prompts (context-cache fill included), captured and replayed."""
    import svi_hip
    models, lat, cp, cn = clip_pair()
    outs = []
    for m in models:
        loop = svi_hip.DenoiseLoop(m, graph=True)
        outs.append(loop.sample(lat, cp, cn, num_inference_steps=3))
        assert loop.captures >= 1
    assert torch.isfinite(outs[0].float()).all() and torch.equal(outs[0], outs[1])


def test_graphed_teacache_clip():
    """Eight steps with TeaCache at a threshold that mixes computed and skipped steps (the store and the skip form of the pair forward)."""
    import svi_hip
    models, lat, cp, cn = clip_pair()
    outs, counts = [], []
    for m in models:
        loop = svi_hip.DenoiseLoop(m, graph=True)
        outs.append(loop.sample(lat, cp, cn, num_inference_steps=8, tea_cache_l1_thresh=TEA_THRESH, tea_cache_model_id=synth.TEA_MODEL))
        counts.append(dict(loop.tea_counts))
    assert counts[0] == counts[1] and counts[0]["skipped"] >= 1 and counts[0]["computed"] >= 2, counts          # both forms of the pair forward ran
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("grid", [synth.TALK_GRID, (3, 3, 5)], ids=lambda g: "x".join(map(str, g)))          # 72 tokens; 45 (no multiple of 8: V^T's ragged edge)
def test_forward_talk3(grid):
    """The tiny talk model: the audio projections bound as e4m3 (q_linear, proj, and kv_linear with its V half at a byte offset, K = 768), the three guidance
    forwards as one call on staged audio slots."""
    c, seed = synth.TINY_DIT_TALK, synth.TALK_SEED
    sd = {k: torch.from_numpy(v).to(torch.float8_e4m3fn) for k, v in synth.dit_state_dict(seed, **c).items()}
    f, h, w = grid
    assert_plans_to_128(c, grid, 20, extra_rows=(f * 32, 3 * f * h * w))
    x = dev(synth.randn(seed + 1, 1, 16, f, 2 * h, 2 * w))
    pos, neg = dev(synth.text_context(seed + 2, 20, c["text_dim"], 13)), dev(synth.text_context(seed + 12, 20, c["text_dim"], 4))
    kw = dict(clip_feature=dev(synth.randn(seed + 3, 1, 257, 1280)), y=dev(synth.randn(seed + 4, 1, 20, f, 2 * h, 2 * w)))
    aud, null = (tuple(dev(a) for a in synth.audio_windows(seed + k, f)) for k in (5, 7))
    add = dev(0.5 * synth.randn(seed + 9, 1, f * h * w, c["dim"]))
    outs = []
    for resident in (True, False):
        m = build(c, sd, resident)
        if resident:
            names = listed(m)
            assert len(names) == (10 + (2 if c["has_image_input"] else 0) + 3) * c["num_layers"] and all(m._params[k].dtype == torch.float8_e4m3fn for k in names)
            assert any("audio_cross_attn.kv_linear" in k for k in names)
        m.stage_audio(0, aud)
        m.stage_audio(1, null)
        outs.append([t.clone() for t in m.forward_talk3(x, torch.tensor([637.5]), pos, neg, add_condition=add, **kw)])
    assert all(torch.isfinite(t.float()).all() for t in outs[0])
    for name, a, b in zip(("cond", "uncond", "drop_text"), *outs):
        assert torch.equal(a, b), name


SP_DIT = dict(dim=512, in_dim=16, ffn_dim=1024, out_dim=16, text_dim=64, freq_dim=256, patch_size=(1, 2, 2), num_layers=2, has_image_input=False)


@pytest.mark.parametrize("grid", [(2, 4, 6), (3, 5, 14)], ids=lambda g: "x".join(map(str, g)))          # 48 tokens; 210 (odd shard lengths)
def test_two_sequence_parallel_shards(grid):
    """Two in-process shards (four heads), each handle bound on the same stored tensors: the shard forward and the stacked CFG pair on shards."""
    import svi_hip
    from svi_hip import sequence_parallel as sp
    c = SP_DIT
    f, h, w = grid
    tokens = f * h * w
    assert_plans_to_128(c, grid, 24, extra_rows=(tokens // 2, tokens))
    sd = {k: torch.from_numpy(v).to(torch.float8_e4m3fn).cuda().contiguous() for k, v in synth.dit_state_dict(900, **c).items()}
    x = dev(synth.randn(901, 1, 16, f, 2 * h, 2 * w))
    ca, cb = dev(synth.text_context(902, 24, 64, 17)), dev(synth.text_context(903, 24, 64, 9))
    t = torch.tensor([712.5])
    outs = []
    for resident in (True, False):
        ms = []
        for _ in range(2):
            m = svi_hip.WanDiT(eps=1e-6, num_heads=synth.num_heads_of(c), **c)
            m.bind(sd, fp8_resident=resident)
            ms.append(m)
        assert (ms[0].weight_bytes()["e4m3"] > 0) == resident
        one = sp.forward_local(ms, x, t, ca).clone()
        for m in ms:
            m.context_cache(True)          # the stacked pair keeps each prompt's K / V in buffers of their own
        pa, pb = sp.forward_local_pair(ms, x, t, ca, cb)
        outs.append((one.clone(), pa.clone(), pb.clone()))
    assert all(torch.isfinite(o.float()).all() for o in outs[0])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert torch.equal(outs[0][0], outs[0][1])          # the pair's first branch is the single forward on the same prompt

