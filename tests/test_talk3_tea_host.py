"""Without a GPU: svi_dit_forward_talk3_tea at the C-ABI boundary, the rule by which install()'s talk sampler serves a clip that carries TeaCache objects,
and the host side of the talk loop's TeaCache step — the order of the three checks, the graph key per mode triple, the bound on the graphs kept."""
import ctypes as C
import os
import re
import types

import torch

from conftest import ROOT
from svi_hip import _lib as L

HEADER = os.path.join(ROOT, "include", "svi_hip.h")


def _declaration(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"svi_status\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
    assert m, f"{name} is not declared in svi_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_talk3_tea_symbol_is_declared_exported_and_bound():
    table = {n: (r, a) for n, r, a in L.SYMBOLS}
    lib = L.lib()
    i32, vp = C.c_int32, C.c_void_p
    name, argtypes = "svi_dit_forward_talk3_tea", [vp] * 11 + [i32] * 7 + [vp] * 4
    decl = _declaration(name)
    assert hasattr(lib, name), f"{name} is not exported by libsvi_hip.so"
    assert name in table and table[name][0] is i32 and table[name][1] == argtypes
    assert len(decl) == len(argtypes), decl
    for d, t in zip(decl, argtypes):
        assert d.startswith("int32_t ") == (t is i32), d
    # svi_dit_forward_talk3's arguments, then a mode per branch and a residual per branch, then the stream
    assert decl[:15] == _declaration("svi_dit_forward_talk3")[:15]
    assert decl[15:] == ["int32_t tea_cond", "int32_t tea_uncond", "int32_t tea_drop_text", "void* residual_cond", "void* residual_uncond",
                         "void* residual_drop_text", "svi_stream stream"]
    assert lib.svi_abi_version() == 13


def test_refused_without_a_device():
    lib = L.lib()
    fn = lib.svi_dit_forward_talk3_tea
    assert fn(None, None, None, None, None, None, None, None, None, None, None, 1, 2, 2, 8, 1, 1, 1, None, None, None, None) != 0
    assert "null argument" in L.last_error()
    cfg = L.DitConfig(128, 16, 256, 16, 64, 256, 1e-6, 1, 2, 2, 1, 2, 0, 1)
    h = C.c_void_p()
    assert lib.svi_dit_create(C.byref(cfg), C.byref(h)) == 0
    buf = torch.zeros(4096, dtype=torch.bfloat16)          # host memory: nothing here may get as far as reading it
    p = buf.data_ptr()
    call = lambda modes, res, out=p: fn(h, p, p, p, p, None, None, None, out, p + 2048, p + 4096, 1, 2, 2, 8, *modes, *res, None)      # noqa: E731
    assert call((1, 1, 1), (p, p, p), out=None) != 0 and "null output" in L.last_error()
    for k, arg in enumerate(("tea_cond", "tea_uncond", "tea_drop_text")):
        for bad in (3, -1):
            modes = [1, 1, 1]
            modes[k] = bad
            assert call(modes, (p, p, p)) != 0 and f"{arg} = {bad}" in L.last_error(), L.last_error()
    for k, arg in enumerate(("residual_cond", "residual_uncond", "residual_drop_text")):
        for mode in (1, 2):
            modes, res = [0, 0, 0], [None, None, None]
            modes[k] = mode
            assert call(modes, res) != 0 and f"needs {arg}" in L.last_error(), L.last_error()
        res = [p, p, p]
        res[k] = p + 2
        assert call((2, 2, 2), res) != 0 and f"{arg} must be 16-byte aligned" in L.last_error(), L.last_error()
    assert lib.svi_dit_destroy(h) == 0


def test_sampler_serves_teacache_only_when_nothing_else_passes_through():
    from svi_hip.pipeline import _talk_sampler_passes_through as through, _talk_sampler_serves_tea as serves, _talk_sampler_tea
    hip, P, N = object(), object(), object()
    lat = types.SimpleNamespace(is_cuda=True, dtype=torch.bfloat16)
    base = dict(hip=hip, latents=lat, prompt_emb_posi={"context": 1}, prompt_emb_nega={"context": 2}, image_emb={"clip_feature": 3, "y": 4}, extra_input={},
                tea_cache_posi={"tea_cache": P}, tea_cache_nega={"tea_cache": N}, usp_kwargs={}, use_controlnet=False,
                cfg_scale={"text": 5.0, "audio": 4.0})
    assert serves(**base) is True and through(**base) is True          # the pass-through rule keeps its answer: TeaCache objects pass through
    assert _talk_sampler_tea(base["tea_cache_posi"], base["tea_cache_nega"]) == (P, N)
    assert serves(**dict(base, tea_cache_nega={"tea_cache": None})) is True and serves(**dict(base, tea_cache_posi=None)) is True
    assert _talk_sampler_tea(None, {"tea_cache": N}) == (None, N) and _talk_sampler_tea({"tea_cache": None}, None) is None
    # no object: nothing to serve here, the plain rule decides (and lets the clip through to the fast loop)
    none = dict(base, tea_cache_posi={"tea_cache": None}, tea_cache_nega={"tea_cache": None})
    assert serves(**none) is False and through(**none) is False
    assert serves(**dict(base, tea_cache_nega={"tea_cache": P})) is False          # one object for both sides stays with the pipeline's loop
    for over in (dict(hip=None), dict(use_controlnet=True), dict(usp_kwargs={"use_unified_sequence_parallel": True}), dict(extra_input={"motion": 1}),
                 dict(latents=types.SimpleNamespace(is_cuda=False, dtype=torch.bfloat16)), dict(latents=torch.zeros(1, dtype=torch.bfloat16)),
                 dict(latents=types.SimpleNamespace(is_cuda=True, dtype=torch.float32)), dict(prompt_emb_posi={"context": 1, "extra": 2}),
                 dict(prompt_emb_nega={}), dict(image_emb={"clip_feature": 3, "pose": 5}), dict(cfg_scale={"text": 1.0, "audio": 1.0})):
        assert serves(**dict(base, **over)) is False and through(**dict(base, **over)) is True, over


def test_pass_through_rule_keeps_its_answers():
    """Every case of tests/test_talk3_host.py::test_talk_sampler_pass_through_rule, unchanged."""
    from svi_hip.pipeline import _talk_sampler_passes_through as through
    hip = object()
    lat = types.SimpleNamespace(is_cuda=True, dtype=torch.bfloat16)
    base = dict(hip=hip, latents=lat, prompt_emb_posi={"context": 1}, prompt_emb_nega={"context": 2}, image_emb={"clip_feature": 3, "y": 4}, extra_input={},
                tea_cache_posi={"tea_cache": None}, tea_cache_nega={"tea_cache": None}, usp_kwargs={}, use_controlnet=False,
                cfg_scale={"text": 5.0, "audio": 4.0})
    assert through(**base) is False
    assert through(**dict(base, image_emb={})) is False and through(**dict(base, usp_kwargs=None, tea_cache_posi=None, tea_cache_nega=None)) is False
    assert through(**dict(base, cfg_scale={"text": 1.0, "audio": 4.0})) is False and through(**dict(base, cfg_scale={"text": 5.0, "audio": 1.0})) is False
    for over in (dict(hip=None), dict(tea_cache_posi={"tea_cache": object()}), dict(tea_cache_nega={"tea_cache": object()}), dict(use_controlnet=True),
                 dict(usp_kwargs={"use_unified_sequence_parallel": True}), dict(extra_input={"motion": 1}),
                 dict(latents=types.SimpleNamespace(is_cuda=False, dtype=torch.bfloat16)), dict(latents=torch.zeros(1, dtype=torch.bfloat16)),
                 dict(latents=types.SimpleNamespace(is_cuda=True, dtype=torch.float32)), dict(prompt_emb_posi={"context": 1, "extra": 2}),
                 dict(prompt_emb_nega={}), dict(image_emb={"clip_feature": 3, "pose": 5}), dict(cfg_scale={"text": 1.0, "audio": 1.0})):
        assert through(**dict(base, **over)) is True, over


class RecordingDiT:
    """What the talk loop's host side asks of a WanDiT, on the CPU, with a record of the order of events."""
    dim = 8

    def __init__(self, events):
        self.events = events

    def time_mod(self, timestep):
        self.events.append("time_mod")
        return torch.zeros((1, 6, self.dim), dtype=torch.bfloat16)

    def tokens(self, T, H, W):
        return T * (H // 2) * (W // 2)

    def forward_talk3(self, *a, **k):
        self.events.append(("forward_talk3", k.get("tea_modes")))

    def _refresh_if_weights_changed(self):
        pass

    def epoch(self):
        return 0

    def generation(self):
        return 0


class Scripted:
    def __init__(self, name, answers, events):
        self.name, self.answers, self.events, self.n = name, list(answers), events, 0
        self.previous_residual = self.previous_hidden_states = None

    def check(self, dit, x, t_mod):
        self.events.append(("check", self.name))
        self.n += 1
        return self.answers[self.n - 1]


def _loop(events):
    import svi_hip
    loop = svi_hip.DenoiseLoop(RecordingDiT(events), graph=True)
    lat = torch.zeros((1, 16, 3, 8, 12), dtype=torch.bfloat16)
    loop._cond, loop._uncond, loop._drop = (torch.zeros_like(lat) for _ in range(3))
    return loop, lat


def test_three_checks_in_the_order_p_n_n_before_the_call():
    import pytest
    events = []
    loop, lat = _loop(events)
    ctx = torch.zeros((1, 20, 64), dtype=torch.bfloat16)
    seen = []

    def replay_or_capture(slot, key, tensors, device, timestep, run, bound=2, lru=False):
        seen.append((slot, key, bound, lru))
        run(timestep)
    loop._replay_or_capture = replay_or_capture
    P, N = Scripted("P", [False, True, False], events), Scripted("N", [False, True, True, True, True, False], events)
    ts = torch.zeros(1)
    want_modes = [(1, 1, 2), (2, 2, 2), (1, 2, 1)]
    for i, want in enumerate(want_modes):
        del events[:]
        modes, residuals = loop._talk_tea_decide(lat, ts, P, N)
        assert modes == want
        assert events == ["time_mod", ("check", "P"), ("check", "N"), ("check", "N")]          # all three decisions, in the reference's order
        loop._talk3_graphed(lat, ts, ctx, ctx.clone(), {}, (modes, residuals))
        assert events[-1] == ("forward_talk3", want) and events.index(("forward_talk3", want)) == 4          # ... and all of them before the step's call
        # a computing branch stores into the loop's tensor of its cache — one for P, one for N — and a skipping one reads the cache's previous_residual
        assert residuals[1] is residuals[2] and residuals[0] is not residuals[1]
        assert P.previous_residual is residuals[0] and N.previous_residual is residuals[1]
    from svi_hip.pipeline import TALK_TEA_GRAPHS
    slots, keys = [s[0] for s in seen], [s[1] for s in seen]
    assert slots == [("talk3",) + m for m in want_modes] and len(set(keys)) == 3          # the triple is in the slot AND in the key
    assert all(s[2] == TALK_TEA_GRAPHS and s[3] is True for s in seen)
    assert loop.talk_tea_counts == {m: 1 for m in want_modes} and loop.tea_counts == {"computed": 2, "skipped": 1}
    # the same triple with another residual tensor is another key
    other = (residuals[0].clone(), residuals[1], residuals[2])
    loop._talk3_graphed(lat, ts, ctx, ctx.clone(), {}, (want_modes[-1], other))
    assert seen[-1][0] == seen[-2][0] and seen[-1][1] != seen[-2][1]
    # one side without an object: mode 0, no residual
    modes, residuals = loop._talk_tea_decide(lat, ts, None, Scripted("N", [False, False], events))
    assert modes == (0, 1, 1) and residuals[0] is None
    # a skip before any store is the existing error
    with pytest.raises(RuntimeError, match="skip before any residual was stored"):
        loop._talk_tea_decide(lat, ts, Scripted("P", [True], events), None)


def test_graph_bound_and_lru_eviction():
    from svi_hip.pipeline import TALK_TEA_GRAPHS
    loop, _ = _loop([])
    assert 2 < TALK_TEA_GRAPHS < 8          # more than the pair path's two, fewer than the eight triples two caches can produce
    triples = [(1, 1, 1), (2, 2, 2), (1, 1, 2), (2, 2, 1), (1, 2, 2), (2, 1, 1), (1, 2, 1), (2, 1, 2)]
    for i, t in enumerate(triples):
        slot = ("talk3",) + t
        assert loop._held_graph(slot, lru=True) is None
        loop._keep_tea_graph(slot, dict(n=i), TALK_TEA_GRAPHS)
        assert len(loop._tea_graphs) == min(i + 1, TALK_TEA_GRAPHS)
        if i == 3:                                 # a use of the oldest one saves it from the next eviction
            assert loop._held_graph(("talk3", 1, 1, 1), lru=True) == dict(n=0)
        if i == 4:
            assert ("talk3", 1, 1, 1) in loop._tea_graphs and ("talk3", 2, 2, 2) not in loop._tea_graphs
    assert list(loop._tea_graphs) == [("talk3",) + t for t in triples[-TALK_TEA_GRAPHS:]]
    # the pair path's own bound and order are what they were: two, the oldest capture goes, a look-up is no use
    loop._tea_graphs.clear()
    for s in ((1, 1), (2, 2)):
        loop._keep_tea_graph(s, dict(s=s), 2)
    assert loop._held_graph((1, 1)) == dict(s=(1, 1))
    loop._keep_tea_graph((1, 2), dict(), 2)
    assert list(loop._tea_graphs) == [(2, 2), (1, 2)]
