"""Without a GPU: the talk step's two entry points at the C-ABI boundary, the parameter list of the sampler install() binds over
SVITalkVideoPipeline._sample_with_multitalk, and the rule by which that sampler hands a clip back to the pipeline's own loop."""
import ast
import ctypes as C
import inspect
import os
import re
import types

import pytest
import torch

from conftest import ROOT
from svi_hip import _lib as L

HEADER = os.path.join(ROOT, "include", "svi_hip.h")
REF = os.environ.get("SVI_REFERENCE", "/root/reference")


def _declaration(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"svi_status\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
    assert m, f"{name} is not declared in svi_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_talk3_symbols_are_declared_exported_and_bound():
    table = {n: (r, a) for n, r, a in L.SYMBOLS}
    lib = L.lib()
    i32, vp = C.c_int32, C.c_void_p
    want = {"svi_dit_audio_slot": [vp, i32, vp, vp, i32, vp],
            "svi_dit_forward_talk3": [vp] * 11 + [i32] * 4 + [vp]}
    for name, argtypes in want.items():
        decl = _declaration(name)
        assert hasattr(lib, name), f"{name} is not exported by libsvi_hip.so"
        assert name in table and table[name][0] is i32 and table[name][1] == argtypes, name
        assert len(decl) == len(argtypes), (name, decl)
        for d, t in zip(decl, argtypes):          # int32_t arguments where the table says so, pointers / the stream elsewhere
            assert d.startswith("int32_t ") == (t is i32), (name, d)
    assert _declaration("svi_dit_forward_talk3")[8:11] == ["void* out_cond", "void* out_uncond", "void* out_drop_text"]
    # additions only: the version the other suites pin has not moved
    assert lib.svi_abi_version() == 13


def test_null_handle_is_refused_without_a_device():
    lib = L.lib()
    assert lib.svi_dit_audio_slot(None, 0, None, None, 0, None) != 0 and "null handle" in L.last_error()
    assert lib.svi_dit_forward_talk3(None, None, None, None, None, None, None, None, None, None, None, 1, 2, 2, 8, None) != 0
    assert "null argument" in L.last_error()
    # freeing a slot that was never staged is no error and needs no device
    cfg = L.DitConfig(128, 16, 256, 16, 64, 256, 1e-6, 1, 2, 2, 1, 2, 0, 1)
    h = C.c_void_p()
    assert lib.svi_dit_create(C.byref(cfg), C.byref(h)) == 0
    assert lib.svi_dit_audio_slot(h, 1, None, None, 0, None) == 0
    assert lib.svi_dit_audio_slot(h, 2, None, None, 0, None) != 0 and "slot 2" in L.last_error()
    assert lib.svi_dit_destroy(h) == 0


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "diffsynth")), reason="the reference checkout is not on this box")
def test_talk_sampler_has_the_reference_parameter_list():
    """install() binds _hip_sample_with_multitalk over SVITalkVideoPipeline._sample_with_multitalk: the reference's __call__ passes fourteen arguments
    by position (svi_video_talk.py:552-556), so the two parameter lists must be the same, in order."""
    from svi_hip.pipeline import _hip_sample_with_multitalk
    tree = ast.parse(open(os.path.join(REF, "diffsynth/pipelines/svi_video_talk.py")).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "SVITalkVideoPipeline")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "_sample_with_multitalk")
    ref_params = [a.arg for a in fn.args.args]
    assert not fn.args.kwonlyargs and fn.args.vararg is None and fn.args.kwarg is None and not fn.args.defaults
    assert list(inspect.signature(_hip_sample_with_multitalk).parameters) == ref_params
    call = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "__call__")
    stmt = next(n for n in ast.walk(call) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "_sample_with_multitalk")
    assert len(stmt.args) == len(ref_params) - 1 and not stmt.keywords          # every argument by position


def test_talk_sampler_pass_through_rule():
    from svi_hip.pipeline import _talk_sampler_passes_through as through
    hip = object()
    lat = types.SimpleNamespace(is_cuda=True, dtype=torch.bfloat16)
    base = dict(hip=hip, latents=lat, prompt_emb_posi={"context": 1}, prompt_emb_nega={"context": 2}, image_emb={"clip_feature": 3, "y": 4}, extra_input={},
                tea_cache_posi={"tea_cache": None}, tea_cache_nega={"tea_cache": None}, usp_kwargs={}, use_controlnet=False,
                cfg_scale={"text": 5.0, "audio": 4.0})
    assert through(**base) is False
    assert through(**dict(base, image_emb={})) is False and through(**dict(base, usp_kwargs=None, tea_cache_posi=None, tea_cache_nega=None)) is False
    assert through(**dict(base, cfg_scale={"text": 1.0, "audio": 4.0})) is False and through(**dict(base, cfg_scale={"text": 5.0, "audio": 1.0})) is False
    assert through(**dict(base, usp_kwargs={"use_unified_sequence_parallel": False})) is False
    for over in (dict(hip=None), dict(tea_cache_posi={"tea_cache": object()}), dict(tea_cache_nega={"tea_cache": object()}), dict(use_controlnet=True),
                 dict(usp_kwargs={"use_unified_sequence_parallel": True}), dict(extra_input={"motion": 1}),
                 dict(latents=types.SimpleNamespace(is_cuda=False, dtype=torch.bfloat16)), dict(latents=torch.zeros(1, dtype=torch.bfloat16)),
                 dict(latents=types.SimpleNamespace(is_cuda=True, dtype=torch.float32)), dict(prompt_emb_posi={"context": 1, "extra": 2}),
                 dict(prompt_emb_nega={}), dict(image_emb={"clip_feature": 3, "pose": 5}), dict(cfg_scale={"text": 1.0, "audio": 1.0})):
        assert through(**dict(base, **over)) is True, over


def test_graphed_talk_path_is_the_single_rank_default():
    """DenoiseLoop's rule for the plain step decides for the talk step too: graph=None is on for the single-rank loop, off under a CFG pair or
    sequence parallelism, and an explicit graph=True with either is refused."""
    import svi_hip
    dit = types.SimpleNamespace()
    assert svi_hip.DenoiseLoop(dit).graph and not svi_hip.DenoiseLoop(dit, graph=False).graph
    assert not svi_hip.DenoiseLoop(dit, sequence_parallel=True).graph and not svi_hip.DenoiseLoop(dit, cfg_pair=object()).graph
    with pytest.raises(ValueError, match="single-rank"):
        svi_hip.DenoiseLoop(dit, graph=True, sequence_parallel=True)
    assert svi_hip.DenoiseLoop(dit)._drop is None and callable(svi_hip.DenoiseLoop._sample_talk3)
