"""FP8-resident weights without a GPU: the new C symbols, the e4m3 launch planner, the SVI_FP8_RESIDENT default and the bind keywords."""
import ctypes as C
import inspect
import itertools
import re

from conftest import ROOT
from svi_hip import _lib as L

NEW = ("svi_gemm_bf16_w8", "svi_gemm_w8_plan", "svi_gemm_bf16_skinny")


def test_new_symbols_are_declared_exported_and_typed():
    header = open(f"{ROOT}/include/svi_hip.h").read()
    table = {n: a for n, _, a in L.SYMBOLS}
    for n in NEW:
        assert re.search(rf"\b{n}\s*\(", header), n
        assert hasattr(L.lib(), n), n
    assert re.search(r"\bSVI_E4M3\s*=\s*3\b", header) and L.SVI_E4M3 == 3
    assert table["svi_gemm_bf16_w8"] == table["svi_gemm_bf16_pair"]          # the pair launch's arguments, W / W2 as bytes
    assert table["svi_gemm_w8_plan"] == table["svi_gemm_plan"]


def w8_plan(M, N, K, epi=0, skinny=False, cus=256):
    k = C.c_int32(-1)
    assert L.lib().svi_gemm_w8_plan(M, N, K, epi, 1 if skinny else 0, cus, C.byref(k)) == 0, L.last_error()
    return k.value


def test_w8_plan_names_only_kernels_with_an_e4m3_form():
    """Ids 0 and 128 have one; wherever svi_gemm_plan names one of them the e4m3 launch takes the same, everything else maps to 128."""
    seen = set()
    for M, N, K, epi, skinny in itertools.product((1, 16, 128, 129, 2560, 32760), (8, 136, 1536, 5120, 8960), (64, 72, 128, 1536, 8960), (0, 1, 2), (False, True)):
        b, w = L.gemm_plan(M, N, K, epi, skinny=skinny), w8_plan(M, N, K, epi, skinny)
        seen.add(b)
        assert w in (0, 128), (M, N, K, epi, skinny, w)
        assert w == (b if b in (0, 128) else 128), (M, N, K, epi, skinny, b, w)
    assert {0, 128, 260} <= seen          # the sweep reaches the skinny kernel, the 128^2 tile and the 256^2 tile
    assert L.lib().svi_gemm_w8_plan(0, 8, 8, 0, 0, 256, C.byref(C.c_int32())) != 0 and "svi_gemm_w8_plan" in L.last_error()


def test_dit_weight_slots_that_take_e4m3():
    """The Linear weights inside blocks.* accept SVI_E4M3; norms, biases, modulation, embedders and the head are refused with a message."""
    cfg = L.DitConfig(128, 16, 256, 16, 64, 256, 1e-6, 1, 2, 2, 1, 2, 0, 1)          # multitalk on: the audio projections are there
    h = C.c_void_p()
    assert L.lib().svi_dit_create(C.byref(cfg), C.byref(h)) == 0

    def bind(name, *shape, dtype=L.SVI_E4M3):
        return L.lib().svi_dit_bind_weight(h, name.encode(), 16, dtype, (C.c_int64 * len(shape))(*shape), len(shape))
    for mod in ("self_attn.q", "self_attn.k", "self_attn.v", "self_attn.o", "cross_attn.q", "cross_attn.k", "cross_attn.v", "cross_attn.o",
                "audio_cross_attn.q_linear", "audio_cross_attn.proj"):
        assert bind(f"blocks.1.{mod}.weight", 128, 128) == 0, (mod, L.last_error())
        assert bind(f"blocks.1.{mod}.weight", 128, 128, dtype=L.SVI_BF16) == 0          # and back: a handle may mix
    assert bind("blocks.0.ffn.0.weight", 256, 128) == 0 and bind("blocks.0.ffn.2.weight", 128, 256) == 0
    assert bind("blocks.0.audio_cross_attn.kv_linear.weight", 256, 768) == 0
    for name, shape in (("blocks.0.self_attn.q.bias", (128,)), ("blocks.0.self_attn.norm_q.weight", (128,)), ("blocks.0.modulation", (1, 6, 128)),
                        ("head.head.weight", (64, 128)), ("text_embedding.0.weight", (128, 64)), ("time_embedding.0.weight", (128, 256))):
        assert bind(name, *shape) == 1 and "must be bf16" in L.last_error(), name
        assert bind(name, *shape, dtype=L.SVI_BF16) == 0, (name, L.last_error())
    assert L.lib().svi_dit_destroy(h) == 0


def test_e4m3_inner_dimension_is_checked_at_bind():
    """An e4m3 weight whose rows are no multiple of 16 bytes (ffn_dim = 264: ffn.2 is [128, 264]) is refused when it is bound, not at the first launch."""
    cfg = L.DitConfig(128, 16, 264, 16, 64, 256, 1e-6, 1, 2, 2, 1, 2, 0, 0)
    h = C.c_void_p()
    assert L.lib().svi_dit_create(C.byref(cfg), C.byref(h)) == 0
    shape = (C.c_int64 * 2)(128, 264)
    assert L.lib().svi_dit_bind_weight(h, b"blocks.0.ffn.2.weight", 16, L.SVI_E4M3, shape, 2) == 1 and "multiple of 16" in L.last_error()
    assert L.lib().svi_dit_bind_weight(h, b"blocks.0.ffn.2.weight", 16, L.SVI_BF16, shape, 2) == 0
    assert L.lib().svi_dit_bind_weight(h, b"blocks.0.ffn.0.weight", 16, L.SVI_E4M3, (C.c_int64 * 2)(264, 128), 2) == 0
    assert L.lib().svi_dit_destroy(h) == 0


def test_fp8_resident_environment_default(monkeypatch):
    from svi_hip.dit import fp8_resident_default
    monkeypatch.delenv("SVI_FP8_RESIDENT", raising=False)
    assert fp8_resident_default() is False
    for v, want in (("1", True), ("true", True), (" ON ", True), ("yes", True), ("0", False), ("", False), ("2", False), ("off", False)):
        monkeypatch.setenv("SVI_FP8_RESIDENT", v)
        assert fp8_resident_default() is want, v


def test_bind_keywords_default_to_the_environment():
    import svi_hip
    from svi_hip import checkpoint, pipeline
    for fn in (svi_hip.WanDiT.bind, svi_hip.WanDiT.from_state_dict, svi_hip.WanDiT.from_module, checkpoint.load_dit, pipeline.install):
        p = inspect.signature(fn).parameters["fp8_resident"]
        assert p.default is None, fn          # None: SVI_FP8_RESIDENT, else False — today's behaviour
    assert callable(svi_hip.WanDiT.weight_bytes)


def test_resident_key_pattern():
    from svi_hip.dit import _FP8_RESIDENT_KEY as K
    yes = ["blocks.0.self_attn.q.weight", "blocks.39.cross_attn.v_img.weight", "blocks.3.cross_attn.k_img.weight", "blocks.7.ffn.0.weight", "blocks.7.ffn.2.weight",
           "blocks.1.audio_cross_attn.kv_linear.weight", "blocks.1.audio_cross_attn.proj.weight"]
    no = ["blocks.0.self_attn.q.bias", "blocks.0.self_attn.norm_q.weight", "blocks.0.modulation", "blocks.0.norm3.weight", "head.head.weight", "patch_embedding.weight",
          "text_embedding.0.weight", "img_emb.proj.1.weight", "audio_proj.proj1.weight", "blocks.0.ffn.1.weight", "xblocks.0.ffn.0.weight"]
    assert all(K.match(k) for k in yes) and not any(K.match(k) for k in no)
