"""TeaCache on the graphed loop, the parts that need no GPU: the new C entry is declared, exported and typed, the ABI is still v12, and
DenoiseLoop.step()'s mode selection — pair call / one call per branch, which captured graph serves the step — on a fake WanDiT that records calls."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT
from svi_hip import _lib as L

HEADER = os.path.join(ROOT, "include", "svi_hip.h")
NAME = "svi_dit_forward_cfg_pair_tea"


def test_pair_tea_entry_is_declared_exported_and_typed():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"svi_status\s+" + NAME + r"\s*\(([^;]*)\)\s*;", src)
    assert m, "not declared in svi_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    want = {"svi_dit*": C.c_void_p, "const void*": C.c_void_p, "void*": C.c_void_p, "const float*": C.c_void_p, "int32_t": C.c_int32, "svi_stream": C.c_void_p}
    declared = [want[p.rsplit(" ", 1)[0]] for p in params]
    assert [p.rsplit(" ", 1)[1] for p in params][-4:] == ["tea_mode", "residual_cond", "residual_uncond", "stream"]
    row = [r for r in L.SYMBOLS if r[0] == NAME]
    assert len(row) == 1 and row[0][1] is C.c_int32 and list(row[0][2]) == declared
    # the plain pair's arguments, then tea_mode and one residual per branch in front of the stream
    plain = [r for r in L.SYMBOLS if r[0] == "svi_dit_forward_cfg_pair"][0]
    assert list(row[0][2]) == list(plain[2][:-1]) + [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    fn = getattr(L.lib(), NAME)                                     # exported by the built library
    assert fn.restype is C.c_int32 and list(fn.argtypes) == declared
    assert fn(*([None] * 10), 1, 1, 1, 1, 1, 1, None, None, None) == 1 and "null argument" in L.last_error()      # host-side refusal, no device touched


def test_abi_is_v13():
    m = re.search(r"#define\s+SVI_HIP_ABI_VERSION\s+(\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == 13 and L.lib().svi_abi_version() == 13


# ---- step()'s mode selection ---------------------------------------------------------------------------------------------------------
class FakeDiT:
    dim, patch_size, has_image_input, _ctx_cache_on = 8, (1, 2, 2), False, True

    def __init__(self):
        self.calls = []

    def tokens(self, T, H, W):
        return T * (H // 2) * (W // 2)

    def time_mod(self, timestep):
        return timestep.reshape(-1, 1, 1).expand(-1, 6, self.dim).to(torch.bfloat16)

    def epoch(self):
        return 0

    def forward(self, x, t, ctx, out=None, tea_mode=0, residual=None, **kw):
        self.calls.append(("one", tea_mode, residual, sorted(k for k, v in kw.items() if v is not None)))

    def forward_cfg_pair(self, x, t, cp, cn, out_cond=None, out_uncond=None, tea_mode=0, residual_cond=None, residual_uncond=None, **kw):
        self.calls.append(("pair", tea_mode, residual_cond, residual_uncond))


class Scripted:
    """A TeaCache that takes the decisions it is told (True = skip)."""
    def __init__(self, skips):
        self.skips, self.previous_residual, self.previous_hidden_states, self.seen = list(skips), None, "untouched", []

    def check(self, dit, x, t_mod):
        self.seen.append((tuple(x.shape), tuple(t_mod.shape)))
        return self.skips.pop(0)


@pytest.fixture
def loop(monkeypatch):
    from svi_hip import pipeline
    monkeypatch.setattr(pipeline.ops, "cfg_step_", lambda *a, **k: None)
    lp = pipeline.DenoiseLoop(FakeDiT(), graph=True)
    assert lp.tea_graph
    lp.graph = False                     # the forwards run as they would be recorded; capture itself needs a device (tests/test_gpu_teacache_graph.py)
    return lp


def _inputs(nt_neg=5):
    return torch.zeros((1, 16, 2, 4, 4), dtype=torch.bfloat16), torch.tensor([500.0]), torch.zeros((1, 5, 4), dtype=torch.bfloat16), torch.zeros((1, nt_neg, 4), dtype=torch.bfloat16)


def test_step_takes_the_pair_when_the_caches_agree(loop):
    lat, t, cp, cn = _inputs()
    tp, tn = Scripted([False, True, True]), Scripted([False, True, True])
    for _ in range(3):
        loop.step(lat, t, -0.1, cp, cn, 5.0, tea_cache_posi=tp, tea_cache_nega=tn)
    calls = loop.dit.calls
    assert [c[:2] for c in calls] == [("pair", 1), ("pair", 2), ("pair", 2)]
    rc, ru = calls[0][2], calls[0][3]
    assert tuple(rc.shape) == (1, 8, 8) and rc.dtype == torch.bfloat16 and rc is not ru
    assert calls[1][2] is rc and calls[1][3] is ru                   # a skip adds what the store left: the objects' previous_residual
    assert tp.previous_residual is rc and tn.previous_residual is ru and tp.previous_hidden_states is None
    assert tp.seen[0] == ((1, 1, 1), (1, 6, 8))                       # check(dit, token, t_mod): the decision is the object's own
    assert loop.tea_counts == {"computed": 1, "skipped": 2}
    # the graph that serves a step: one slot per mode, the residuals' identities in the key, the plain step's key without either
    s1, k1, pins1 = loop._graph_key(lat, cp, cn, 5.0, False, {}, (1, rc, 1, ru))
    s2, k2, _ = loop._graph_key(lat, cp, cn, 5.0, False, {}, (2, rc, 2, ru))
    s0, k0, pins0 = loop._graph_key(lat, cp, cn, 5.0, False, {}, None)
    assert (s1, s2, s0) == ((1, 1), (2, 2), None) and len({k1, k2, k0}) == 3 and k1[:len(k0)] == k0
    assert any(p is rc for p in pins1) and not any(p is rc for p in pins0)
    assert loop._graph_key(lat, cp, cn, 5.0, False, {}, (1, rc.clone(), 1, ru))[1] != k1
    assert loop._graph_key(lat, cp, cn, 5.0, False, {}, (1, rc, 1, ru))[1] == k1


def test_step_takes_one_call_per_branch_otherwise(loop):
    lat, t, cp, cn = _inputs()
    add = torch.zeros((1, 8, 8), dtype=torch.bfloat16)
    # the dance variant: add_condition on the conditional branch only
    tp, tn = Scripted([False, True]), Scripted([False, True])
    for _ in range(2):
        loop.step(lat, t, -0.1, cp, cn, 5.0, tea_cache_posi=tp, tea_cache_nega=tn, add_condition=add)
    assert [(c[0], c[1], c[3]) for c in loop.dit.calls] == [("one", 1, ["add_condition"]), ("one", 1, []), ("one", 2, ["add_condition"]), ("one", 2, [])]
    assert loop.dit.calls[2][2] is tp.previous_residual and loop.dit.calls[3][2] is tn.previous_residual
    # caches that disagree: each branch in its own mode
    loop.dit.calls.clear()
    tp, tn = Scripted([False, False]), Scripted([False, True])
    for _ in range(2):
        loop.step(lat, t, -0.1, cp, cn, 5.0, tea_cache_posi=tp, tea_cache_nega=tn)
    assert [c[:2] for c in loop.dit.calls] == [("pair", 1), ("one", 1), ("one", 2)]
    assert loop._graph_key(lat, cp, cn, 5.0, False, {}, (1, tp.previous_residual, 2, tn.previous_residual))[0] == (1, 2)
    # prompts of unequal shapes; no guidance (one branch, the unconditional cache is not consulted); no cache for the unconditional branch
    loop.dit.calls.clear()
    lat, t, cp, cn6 = _inputs(6)
    loop.step(lat, t, -0.1, cp, cn6, 5.0, tea_cache_posi=Scripted([False]), tea_cache_nega=Scripted([False]))
    idle = Scripted([False])
    loop.step(lat, t, -0.1, cp, None, 1.0, tea_cache_posi=Scripted([False]), tea_cache_nega=idle)
    loop.step(lat, t, -0.1, cp, cn, 5.0, tea_cache_posi=Scripted([False]), tea_cache_nega=None)
    assert [c[:2] for c in loop.dit.calls] == [("one", 1), ("one", 1), ("one", 1), ("one", 1), ("one", 0)] and idle.seen == []


def test_a_skip_before_any_store_raises_and_graph_false_keeps_the_eager_path(loop, monkeypatch):
    from svi_hip import pipeline
    lat, t, cp, cn = _inputs()
    with pytest.raises(RuntimeError, match="before any residual"):
        loop.step(lat, t, -0.1, cp, cn, 5.0, tea_cache_posi=Scripted([True]), tea_cache_nega=Scripted([True]))
    assert loop.dit.calls == []
    # graph=False: the two forwards go through model_fn_wan_video, as before; graph=None follows the module's default
    seen = []
    monkeypatch.setattr(pipeline, "model_fn_wan_video", lambda dit, x, ts, ctx, tea_cache=None, **kw: seen.append(tea_cache))
    monkeypatch.setattr("svi_hip.dit.model_fn_wan_video", pipeline.model_fn_wan_video)
    eager = pipeline.DenoiseLoop(FakeDiT(), graph=False)
    tp, tn = Scripted([]), Scripted([])
    eager.step(lat, t, -0.1, cp, cn, 5.0, tea_cache_posi=tp, tea_cache_nega=tn)
    assert seen == [tp, tn] and eager.dit.calls == [] and not eager.tea_graph
    assert pipeline.DenoiseLoop(FakeDiT()).tea_graph == pipeline.TEA_GRAPH_BY_DEFAULT
    with pytest.raises(ValueError):
        pipeline.DenoiseLoop(FakeDiT(), graph=True, sequence_parallel=True)
