"""-m gpu: TeaCache steps on the graphed, resident, pair-sharing path (DenoiseLoop(graph=True) + tea_cache_l1_thresh).

The acceptance is bit-identity: the operator seam svi_dit_forward_cfg_pair_tea against two svi_dit_forward_tea calls, and the graphed loop against the
eager TeaCache loop (DenoiseLoop(graph=False): the forwards of a step through model_fn_wan_video, one by one).  Shapes are tests/test_teacache.py's:
the tiny DiTs, grid (3, 4, 6), 20 prompt tokens.

Thresholds: the tiny models' random time embedding moves t_mod by O(1) between the 8 steps of the schedule, where the TeaCache polynomial (fitted for
relative changes of a few per cent) is hugely NEGATIVE — about -1e4 .. -3e4 per step — so any positive threshold skips every middle step.  A mixed
pattern therefore needs a negative threshold: at MIXED_THRESH the small early increments compute and the larger late ones skip.  The tests read the
pattern from loop.tea_counts and pin no list."""
import numpy as np
import pytest
import torch

import synth
from gpu_util import dev, report

pytestmark = pytest.mark.gpu

GRID, NT, NV = (3, 4, 6), 20, 13
STEPS, MIXED_THRESH = 8, -2.0e4


def build(c, seed):
    import svi_hip
    sd = {k: torch.from_numpy(v) for k, v in synth.dit_state_dict(seed, **c).items()}
    return svi_hip.WanDiT.from_state_dict(sd, eps=1e-6, num_heads=synth.num_heads_of(c), **c)


def clip_inputs(c, seed, grid=GRID, B=1, add=False):
    f, h, w = grid
    lat = dev(synth.randn(seed + 1, B, 16, f, 2 * h, 2 * w))
    cp = dev(np.concatenate([synth.text_context(seed + 2 + 10 * b, NT, c["text_dim"], NV) for b in range(B)]))
    cn = dev(np.concatenate([synth.text_context(seed + 3 + 10 * b, NT, c["text_dim"], NV - 4) for b in range(B)]))
    kw = {}
    if c["has_image_input"]:
        kw["clip_feature"] = dev(synth.randn(seed + 4, B, 257, 1280))
        kw["y"] = dev(synth.randn(seed + 5, B, c["in_dim"] - 16, f, 2 * h, 2 * w))
    if add:
        kw["add_condition"] = dev(0.1 * synth.randn(seed + 6, B, f * h * w, c["dim"]))
    return lat, cp, cn, kw


@pytest.fixture(scope="module")
def t2v():
    """The T2V tiny model, one clip's inputs and the eager TeaCache loop's latents at MIXED_THRESH — computed once, never modified."""
    import svi_hip
    m = build(synth.TINY_DIT, 100)
    lat, cp, cn, _ = clip_inputs(synth.TINY_DIT, 100)
    eager = svi_hip.DenoiseLoop(m, graph=False)
    want = eager.sample(lat, cp, cn, num_inference_steps=STEPS, tea_cache_l1_thresh=MIXED_THRESH, tea_cache_model_id=synth.TEA_MODEL)
    return dict(m=m, lat=lat, cp=cp, cn=cn, want=want)


class Arena:
    """A residual buffer between NaN guard rows."""
    G = 3

    def __init__(self, B, L, D):
        self.all = torch.full((2 * self.G + B * L, D), float("nan"), dtype=torch.bfloat16, device="cuda")
        self.res = self.all[self.G:self.G + B * L].view(B, L, D)
        self.res.fill_(7.0)

    def guards_intact(self):
        return bool(torch.isnan(self.all[:self.G]).all() and torch.isnan(self.all[-self.G:]).all())


# ---- 1. operator seam ------------------------------------------------------------------------------------------------------------
# (3, 4, 6): L = 72 — with the context cache the stacked form (one row-kernel launch for both branches, head on 2 L rows); without it the branch-by-branch
# form.  (3, 3, 5): L = 45 is no multiple of 8 (never stacked) nor of the row kernel's 4 rows per workgroup: its last workgroup runs one row.
@pytest.mark.parametrize("model", ["tiny_t2v", "tiny_i2v"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("grid,cache,add", [((3, 4, 6), True, False), ((3, 4, 6), True, True), ((3, 4, 6), False, True), ((3, 3, 5), True, True)])
def test_pair_tea_is_bit_identical_to_two_tea_forwards(model, B, grid, cache, add):
    c, seed = (synth.TINY_DIT, 100) if model == "tiny_t2v" else (synth.TINY_DIT_I2V, 200)
    m = build(c, seed)
    x1, cp, cn, kw = clip_inputs(c, seed, grid, B, add)
    x2 = dev(synth.randn(seed + 7, *x1.shape))                       # the skipped step sees other latents and another timestep
    t1, t2 = torch.tensor([637.5] * B), torch.tensor([601.25] * B)
    L, D = grid[0] * grid[1] * grid[2], c["dim"]
    ra, rb = (torch.full((B, L, D), 7.0, dtype=torch.bfloat16, device="cuda") for _ in range(2))
    m.context_cache(cache)
    try:
        a1 = m.forward(x1, t1, cp, tea_mode=1, residual=ra, **kw).clone()
        b1 = m.forward(x1, t1, cn, tea_mode=1, residual=rb, **kw).clone()
        a2 = m.forward(x2, t2, cp, tea_mode=2, residual=ra, **kw).clone()
        b2 = m.forward(x2, t2, cn, tea_mode=2, residual=rb, **kw).clone()
        A, Bn = Arena(B, L, D), Arena(B, L, D)
        pa1, pb1 = (o.clone() for o in m.forward_cfg_pair(x1, t1, cp, cn, tea_mode=1, residual_cond=A.res, residual_uncond=Bn.res, **kw))
        assert torch.equal(A.res, ra) and torch.equal(Bn.res, rb)
        pa2, pb2 = m.forward_cfg_pair(x2, t2, cp, cn, tea_mode=2, residual_cond=A.res, residual_uncond=Bn.res, **kw)
        # mode 0 through the same entry is the plain pair
        q = m.forward_cfg_pair(x1, t1, cp, cn, **kw)
        p0 = m.forward(x1, t1, cp, **kw)
    finally:
        m.context_cache(False)
    assert torch.equal(pa1, a1) and torch.equal(pb1, b1)
    assert torch.equal(pa2, a2) and torch.equal(pb2, b2)
    assert torch.equal(A.res, ra) and torch.equal(Bn.res, rb)       # the skip reads the residuals, it does not write them
    assert A.guards_intact() and Bn.guards_intact()
    assert torch.equal(q[0], p0) and torch.equal(p0, a1)
    # the case is not vacuous: the branches differ, the residuals differ, a skipped step is not a computed one
    assert not torch.equal(ra, rb) and not torch.equal(a1, b1) and not torch.equal(a2, b2) and torch.isfinite(a2.float()).all()
    assert not torch.equal(a2, m.forward(x2, t2, cp, **kw))


# The skip kernel at the product widths: the tiny models above run it at MAXC = 3 with partly filled lanes only.  Dim 1536 (1.3B) is MAXC = 3 and dim 5120
# (14B) MAXC = 10, every lane full; the two forward(tea_mode=2) calls it is held against run add_bf16 + svi_launch_ln_mod, the multi-row kernel at these
# widths.  (1, 3, 5): L = 15, no multiple of 8 (branch by branch) nor of the 4 rows per workgroup (the last one runs 3); (1, 4, 6) with the context cache:
# L = 24, the stacked form (one launch serves both branches).  One block and narrow ffn / text widths: the models are built once per module.
_WIDE = {}


def wide_model(dim):
    c = dict(dim=dim, in_dim=16, ffn_dim=256, out_dim=16, text_dim=64, freq_dim=256, patch_size=(1, 2, 2), num_layers=1, has_image_input=False)
    if dim not in _WIDE:
        _WIDE[dim] = build(c, 300 + dim)
    return c, _WIDE[dim]


@pytest.mark.parametrize("dim", [1536, 5120])
@pytest.mark.parametrize("grid,cache", [((1, 3, 5), False), ((1, 4, 6), True)])
def test_pair_tea_skip_at_the_product_widths(dim, grid, cache):
    c, m = wide_model(dim)
    seed = 300 + dim
    x1, cp, cn, kw = clip_inputs(c, seed, grid)
    x2 = dev(synth.randn(seed + 7, *x1.shape))
    t1, t2 = torch.tensor([637.5]), torch.tensor([601.25])
    L = grid[0] * grid[1] * grid[2]
    ra, rb = (torch.full((1, L, dim), 7.0, dtype=torch.bfloat16, device="cuda") for _ in range(2))
    m.context_cache(cache)
    try:
        a1 = m.forward(x1, t1, cp, tea_mode=1, residual=ra, **kw).clone()
        b1 = m.forward(x1, t1, cn, tea_mode=1, residual=rb, **kw).clone()
        a2 = m.forward(x2, t2, cp, tea_mode=2, residual=ra, **kw).clone()
        b2 = m.forward(x2, t2, cn, tea_mode=2, residual=rb, **kw).clone()
        A, Bn = Arena(1, L, dim), Arena(1, L, dim)
        pa1, pb1 = (o.clone() for o in m.forward_cfg_pair(x1, t1, cp, cn, tea_mode=1, residual_cond=A.res, residual_uncond=Bn.res, **kw))
        assert torch.equal(A.res, ra) and torch.equal(Bn.res, rb)
        pa2, pb2 = m.forward_cfg_pair(x2, t2, cp, cn, tea_mode=2, residual_cond=A.res, residual_uncond=Bn.res, **kw)
        computed = m.forward(x2, t2, cp, **kw)
    finally:
        m.context_cache(False)
    assert torch.equal(pa1, a1) and torch.equal(pb1, b1)
    assert torch.equal(pa2, a2) and torch.equal(pb2, b2)
    assert torch.equal(A.res, ra) and torch.equal(Bn.res, rb)       # the skip reads the residuals, it does not write them
    assert A.guards_intact() and Bn.guards_intact()
    # not vacuous: the branches differ, the residuals differ, a skipped step is not a computed one
    assert not torch.equal(ra, rb) and not torch.equal(a1, b1) and not torch.equal(a2, b2) and torch.isfinite(a2.float()).all()
    assert not torch.equal(a2, computed)


# ---- 2. refusals -----------------------------------------------------------------------------------------------------------------
def test_pair_tea_refusals():
    from svi_hip import _lib as L
    c = synth.TINY_DIT
    m = build(c, 100)
    x, cp, cn, _ = clip_inputs(c, 100)
    t = torch.tensor([637.5])
    res = torch.zeros((1, 72, c["dim"]), dtype=torch.bfloat16, device="cuda")
    oa, ob = torch.empty_like(x), torch.empty_like(x)
    for mode in (1, 2):
        with pytest.raises(ValueError, match="residual"):
            m.forward_cfg_pair(x, t, cp, cn, tea_mode=mode)
        with pytest.raises(ValueError, match="residual"):
            m.forward_cfg_pair(x, t, cp, cn, tea_mode=mode, residual_cond=res)
        # ... and by the library itself: no buffer, one buffer for both branches
        for r_c, r_u in ((None, None), (res, None), (res, res)):
            st = L.lib().svi_dit_forward_cfg_pair_tea(m._h, L.ptr(x), L.ptr(t.cuda()), L.ptr(cp), L.ptr(cn), None, None, None, L.ptr(oa), L.ptr(ob),
                                                      1, 3, 8, 12, NT, mode, L.ptr(r_c), L.ptr(r_u), L.current_stream())
            assert st == 1 and "residual buffer per branch" in L.last_error()
    st = L.lib().svi_dit_forward_cfg_pair_tea(m._h, L.ptr(x), L.ptr(t.cuda()), L.ptr(cp), L.ptr(cn), None, None, None, L.ptr(oa), L.ptr(ob),
                                              1, 3, 8, 12, NT, 3, L.ptr(res), L.ptr(res), L.current_stream())
    assert st == 1
    # the talk variant armed: the pair's branches differ in their audio — SVI_ERR_UNSUPPORTED (4), the plain pair's message
    ct = synth.TINY_DIT_TALK
    mt = build(ct, 930)
    f, h, w = GRID
    xt = dev(synth.randn(1, 1, 16, f, 2 * h, 2 * w))
    kw = dict(clip_feature=dev(synth.randn(3, 1, 257, 1280)), y=dev(synth.randn(4, 1, 20, f, 2 * h, 2 * w)))
    ctx, neg = dev(synth.text_context(2, 16, 64, 9)), dev(synth.text_context(5, 16, 64, 4))
    rt = [torch.zeros((1, f * h * w, ct["dim"]), dtype=torch.bfloat16, device="cuda") for _ in range(2)]
    mt.set_audio(tuple(dev(a) for a in synth.audio_windows(6, f)))
    try:
        for mode in (1, 2):
            with pytest.raises(RuntimeError, match=r"status 4.*audio"):
                mt.forward_cfg_pair(xt, t, ctx, neg, tea_mode=mode, residual_cond=rt[0], residual_uncond=rt[1], **kw)
    finally:
        mt.set_audio(None)


# ---- 3. loop: graphed == eager -----------------------------------------------------------------------------------------------------
def test_graphed_teacache_loop_has_the_eager_loops_bits(t2v):
    import svi_hip
    m = t2v["m"]
    calls = []
    pair = m.forward_cfg_pair
    m.forward_cfg_pair = lambda *a, **k: (calls.append(k.get("tea_mode", 0)), pair(*a, **k))[1]
    try:
        loop = svi_hip.DenoiseLoop(m, graph=True)
        got = loop.sample(t2v["lat"], t2v["cp"], t2v["cn"], num_inference_steps=STEPS, tea_cache_l1_thresh=MIXED_THRESH, tea_cache_model_id=synth.TEA_MODEL)
    finally:
        del m.forward_cfg_pair
    n = loop.tea_counts
    report("teacache_graph_loop", thresh=MIXED_THRESH, computed=n["computed"], skipped=n["skipped"], captures=loop.captures, calls=str(calls))
    assert n["computed"] + n["skipped"] == STEPS
    assert n["computed"] >= 2 + 2 and n["skipped"] >= 2             # first and last always compute: at least two computed and two skipped middle steps
    assert torch.equal(got, t2v["want"])
    assert loop.captures == 2                                       # one graph per mode; every other step replayed
    assert sorted(calls) == [1, 1, 2, 2]                            # per capture the eager step and its recording, through the PAIR entry
    assert not loop._tea_graphs and loop._graph is None             # the graphs die with the clip
    plain = svi_hip.DenoiseLoop(m, graph=True).sample(t2v["lat"], t2v["cp"], t2v["cn"], num_inference_steps=STEPS)
    assert not torch.equal(plain, got)


# ---- 4. thresholds -------------------------------------------------------------------------------------------------------------------
def test_threshold_extremes_on_the_graphed_loop(t2v):
    import svi_hip
    m, lat, cp, cn = t2v["m"], t2v["lat"], t2v["cp"], t2v["cn"]
    plain = svi_hip.DenoiseLoop(m, graph=True).sample(lat, cp, cn, num_inference_steps=STEPS)
    loop = svi_hip.DenoiseLoop(m, graph=True)
    never = loop.sample(lat, cp, cn, num_inference_steps=STEPS, tea_cache_l1_thresh=-1e30, tea_cache_model_id=synth.TEA_MODEL)
    assert torch.equal(never, plain) and loop.tea_counts == {"computed": STEPS, "skipped": 0} and loop.captures == 1
    loop = svi_hip.DenoiseLoop(m, graph=True)
    always = loop.sample(lat, cp, cn, num_inference_steps=STEPS, tea_cache_l1_thresh=1e30, tea_cache_model_id=synth.TEA_MODEL)
    assert loop.tea_counts == {"computed": 2, "skipped": STEPS - 2} and loop.captures == 2
    want = svi_hip.DenoiseLoop(m, graph=False).sample(lat, cp, cn, num_inference_steps=STEPS, tea_cache_l1_thresh=1e30, tea_cache_model_id=synth.TEA_MODEL)
    assert torch.equal(always, want) and not torch.equal(always, plain)


# ---- 5. resident stream ----------------------------------------------------------------------------------------------------------------
def test_resident_loop_stays_resident_with_teacache():
    import svi_hip
    c = synth.TINY_DIT_I2V
    m = build(c, 200)
    clips = [clip_inputs(c, 200 + 50 * k) for k in range(2)]         # equal shapes, other latents / prompts / conditioning
    tea = dict(num_inference_steps=STEPS, tea_cache_l1_thresh=1e30, tea_cache_model_id=synth.TEA_MODEL)
    want = [svi_hip.DenoiseLoop(m, graph=False).sample(lat, cp, cn, **tea, **kw) for lat, cp, cn, kw in clips]
    loop = svi_hip.DenoiseLoop(m, graph=True, resident=True)
    try:
        lat, cp, cn, kw = clips[0]
        assert torch.equal(loop.sample(lat, cp, cn, **tea, **kw), want[0])
        assert loop.captures == 2 and len(loop._tea_graphs) == 2 and m._ctx_cache_on
        gen = m.generation()
        slots = {k: v.data_ptr() for k, v in loop._slots.items()}
        assert {"tea_residual_cond", "tea_residual_uncond"} <= set(slots)
        lat, cp, cn, kw = clips[1]
        assert torch.equal(loop.sample(lat, cp, cn, **tea, **kw), want[1])
        assert loop.captures == 2                                    # no re-capture at the clip boundary
        assert m.generation() == gen and {k: v.data_ptr() for k, v in loop._slots.items()} == slots
        assert loop.tea_counts == {"computed": 2, "skipped": STEPS - 2}
    finally:
        loop.close()
    assert not torch.equal(want[0], want[1])


# ---- 6. the reference's object ---------------------------------------------------------------------------------------------------------
def _drive(loop, lat0, cp, cn, tp, tn, steps=STEPS, cfg=5.0, **kw):
    """The steps of one clip through step(), with the caller's TeaCache objects."""
    loop.scheduler.set_timesteps(steps, shift=5.0)
    ts = loop.scheduler.timesteps.to("cuda", torch.float32)
    lat = lat0.clone()
    loop.dit.context_cache(True)
    try:
        for i, t in enumerate(loop.scheduler.timesteps):
            loop.step(lat, ts[i:i + 1], loop.scheduler.step_delta(t), cp, cn, cfg, tea_cache_posi=tp, tea_cache_nega=tn, **kw)
            yield i, lat
    finally:
        loop.drop_graph()
        loop.dit.context_cache(False)


def test_reference_shaped_object_on_the_graphed_loop(t2v):
    import svi_hip

    class RefLike(svi_hip.TeaCache):
        """The REFERENCE class's interface and bookkeeping (check / previous_residual / previous_hidden_states), as tests/test_teacache.py's duck."""
        def check(self, dit, x, t_mod):
            skip = super().check(dit, x, t_mod)
            if not skip:
                self.previous_hidden_states = x.clone()
            return skip
    m, lat, cp, cn = t2v["m"], t2v["lat"], t2v["cp"], t2v["cn"]
    loop = svi_hip.DenoiseLoop(m, graph=True)
    tp, tn = RefLike(STEPS, MIXED_THRESH, synth.TEA_MODEL), RefLike(STEPS, MIXED_THRESH, synth.TEA_MODEL)
    first = None
    for i, cur in _drive(loop, lat, cp, cn, tp, tn):
        for tc in (tp, tn):
            assert tc.previous_hidden_states is None                 # a computed step clears what check() cloned; a skipped step leaves it
            assert tc.previous_residual is not None and tuple(tc.previous_residual.shape) == (1, 72, 128)
        first = first or (tp.previous_residual, tn.previous_residual)
        assert tp.previous_residual is first[0] and tn.previous_residual is first[1] and first[0] is not first[1]     # the loop's own tensors, one per branch
        last = cur
    assert torch.equal(last, t2v["want"]) and loop.captures == 2
    assert tp.step == 0 and tn.step == 0                             # both objects walked the 8 steps (the counter wrapped)
    # a skip before any store: refused as model_fn_wan_video refuses it
    bad = svi_hip.TeaCache(STEPS, 1e30, synth.TEA_MODEL)
    bad.step = 1
    bad.previous_modulated_input = m.time_mod(torch.tensor([500.0]))
    with pytest.raises(RuntimeError, match="before any residual"):
        svi_hip.DenoiseLoop(m, graph=True).step(lat.clone(), torch.tensor([500.0], device="cuda"), -0.1, cp, cn, 5.0, tea_cache_posi=bad, tea_cache_nega=bad)


# ---- 7. fallbacks ----------------------------------------------------------------------------------------------------------------------
def _spy(m):
    calls = []
    pair, fwd = m.forward_cfg_pair, m.forward
    m.forward_cfg_pair = lambda *a, **k: (calls.append(("pair", k.get("tea_mode", 0))), pair(*a, **k))[1]
    m.forward = lambda *a, **k: (calls.append(("one", k.get("tea_mode", 0))), fwd(*a, **k))[1]
    return calls


def test_dance_step_and_disagreeing_caches_take_the_two_call_form(t2v):
    import svi_hip
    m, lat, cp, cn = t2v["m"], t2v["lat"], t2v["cp"], t2v["cn"]
    add = dev(0.1 * synth.randn(9, 1, 72, 128))
    mk = lambda thr: svi_hip.TeaCache(STEPS, thr, synth.TEA_MODEL)      # noqa: E731
    # (thresholds of the conditional / unconditional cache, step keywords): the dance variant's pose on the conditional branch only; caches that disagree
    for name, thr, kw in (("dance", (MIXED_THRESH, MIXED_THRESH), dict(add_condition=add)), ("disagree", (MIXED_THRESH, 1e30), {})):
        *_, (_, want) = _drive(svi_hip.DenoiseLoop(m, graph=False), lat, cp, cn, mk(thr[0]), mk(thr[1]), **kw)
        want = want.clone()
        loop = svi_hip.DenoiseLoop(m, graph=True)
        calls = _spy(m)
        try:
            *_, (_, got) = _drive(loop, lat, cp, cn, mk(thr[0]), mk(thr[1]), **kw)
        finally:
            del m.forward_cfg_pair, m.forward
        report("teacache_graph_fallback", case=name, captures=loop.captures, calls=str(calls))
        assert torch.equal(got, want), name
        kinds = {k for k, _ in calls}
        if name == "dance":
            assert kinds == {"one"} and loop.captures == 2, calls          # still graphed: one capture per mode
        else:
            assert ("one", 1) in calls and ("one", 2) in calls and 2 <= loop.captures < STEPS, calls      # the steps the caches disagree on run per branch
    assert not torch.equal(want, t2v["want"])


# ---- 8. staleness ------------------------------------------------------------------------------------------------------------------------
def test_a_prompt_edit_recaptures_the_mode_in_use_only(t2v):
    import svi_hip
    m, lat = t2v["m"], t2v["lat"]
    cp, cn = t2v["cp"].clone(), t2v["cn"].clone()
    thr = 1e30                                                        # C S S S S S S C: the edit falls into the run of skipped steps

    def run(loop, edit_at):
        tp, tn = svi_hip.TeaCache(STEPS, thr, synth.TEA_MODEL), svi_hip.TeaCache(STEPS, thr, synth.TEA_MODEL)
        seen = []
        a, b = cp.clone(), cn.clone()
        for i, cur in _drive(loop, lat, a, b, tp, tn):
            seen.append((loop.captures, loop._tea_graphs.get((1, 1)), loop._tea_graphs.get((2, 2))))
            if i == edit_at:
                a.mul_(0.5)                                           # in place: same address, the version counter moves
        return cur.clone(), seen
    want, _ = run(svi_hip.DenoiseLoop(m, graph=False), 3)
    got, seen = run(svi_hip.DenoiseLoop(m, graph=True), 3)
    assert torch.equal(got, want)
    # steps 0 / 1 capture the store and the skip graph, steps 2 / 3 replay; the edit after step 3 makes step 4 — a skipped step — capture the skip graph
    # again, and only that: the store graph is left where it is until a computed step (the last) finds it stale
    assert [s[0] for s in seen[:4]] == [1, 2, 2, 2]
    assert seen[4][0] == 3 and seen[4][1] is seen[3][1] and seen[4][2] is not seen[3][2] and seen[3][1] is not None
    assert seen[7][1] is not seen[3][1] and seen[7][0] > seen[6][0]
    base, _ = run(svi_hip.DenoiseLoop(m, graph=True), -1)
    assert not torch.equal(base, got) and [s[0] for s in _] == [1, 2, 2, 2, 2, 2, 2, 2]
