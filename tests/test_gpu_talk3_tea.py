"""-m gpu: TeaCache on the talk variant's one-call step — svi_dit_forward_talk3_tea (WanDiT.forward_talk3(tea_modes=...)), DenoiseLoop.sample_multitalk
with TeaCache on the graphed, resident path, and install()'s `_hip_sample_with_multitalk` serving clips that carry TeaCache objects.

Shapes are tests/test_gpu_talk3.py's: the tiny talk model on (3, 4, 6), on one frame (audio_latter NULL) and on 45 tokens (no multiple of the row kernel's
four rows per workgroup, nor of 8).  Every comparison is torch.equal within one process: the new path runs the same kernels on the same operands in the
same order as what it replaces — three WanDiT.forward(tea_mode=, residual=) calls with the audio armed, in the order cond, uncond, drop-text, the last two
sharing ONE negative residual buffer, as the reference's loop consults one negative TeaCache object twice per step (svi_video_talk.py:448-466)."""
import itertools
import sys
import types

import pytest
import torch

import synth
from gpu_util import dev, errs

pytestmark = pytest.mark.gpu

CFG, SEED = synth.TINY_DIT_TALK, synth.TALK_SEED
GRIDS = [synth.TALK_GRID, (1, 4, 6), (3, 3, 5)]
TS_OLD, TS = torch.tensor([820.0]), torch.tensor([637.5])      # the step that left the old residuals, and the step under test
TEA_MODEL = "Wan2.1-I2V-14B-480P"
# The tiny model's random time embedding moves t_mod by O(1) per step, where this checkpoint's polynomial gives 4e4 .. 1e5 per step (checked on the CPU
# with the oracle's embed_time on the 8-step schedule): at 1.4e5 the positive cache skips two steps and computes the third, and the negative one, which is
# consulted twice per step and has its forced calls in mid-clip, falls out of step with it — five distinct triples; at 2e5 four.  The tests read what
# happened from the eager run's own record and fail if the inputs stop providing both kinds of step.
TEA_STEPS, TEA_THRESH_MIXED, TEA_THRESH_FOUR = 8, 1.4e5, 2.0e5
_MODELS = {}


def _model(key="a", cfg=CFG):
    import svi_hip
    m = _MODELS.get(key)
    if m is None:
        sd = {k: torch.from_numpy(v) for k, v in synth.dit_state_dict(SEED, **cfg).items()}
        m = _MODELS[key] = svi_hip.WanDiT.from_state_dict(sd, eps=1e-6, num_heads=synth.num_heads_of(cfg), **cfg)
    m.context_cache(False)
    m.set_audio(None)
    m.stage_audio(0, None)
    m.stage_audio(1, None)
    return m


def _clip(grid, k=0, addc=True, dim=CFG["dim"]):
    f, h, w = grid
    s = SEED + 100 * k
    x = dev(synth.randn(s + 1, 1, 16, f, 2 * h, 2 * w))
    pos = dev(synth.text_context(s + 2, 20, CFG["text_dim"], 13))
    neg = dev(synth.text_context(s + 12, 20, CFG["text_dim"], 4))
    kw = dict(clip_feature=dev(synth.randn(s + 3, 1, 257, 1280)), y=dev(synth.randn(s + 4, 1, 20, f, 2 * h, 2 * w)))
    aud = tuple(dev(a) for a in synth.audio_windows(s + 5, f))
    null = tuple(dev(a) for a in synth.audio_windows(s + 7, f))
    add = dev(0.5 * synth.randn(s + 9, 1, f * h * w, dim)) if addc else None
    return x, pos, neg, kw, aud, null, add


SENTINEL = 7.0


def _three_tea_forwards(m, clip, modes, P, N, ts=TS):
    """The reference of the operator: three armed forwards in the order cond, uncond, drop-text; uncond and drop-text share N."""
    x, pos, neg, kw, aud, null, add = clip
    outs = []
    for ctx, audio, a, mode, res in ((pos, aud, add, modes[0], P), (neg, null, None, modes[1], N), (neg, aud, add, modes[2], N)):
        m.set_audio(audio)
        outs.append(m.forward(x, ts, ctx, add_condition=a, tea_mode=mode, residual=res if mode else None, **kw).clone())
    m.set_audio(None)
    return outs


def _prefill(modes, P, N):
    """Buffers the call is about to write, where nothing reads them first, start from a sentinel: a missing store shows."""
    if modes[0] == 1:
        P.fill_(SENTINEL)
    if modes[1] == 1 or (modes[1] == 0 and modes[2] == 1):
        N.fill_(SENTINEL)


TRIPLES = [t for t in itertools.product((0, 1, 2), repeat=3) if any(t)]          # the eight of {1, 2}^3 and the eighteen with a 0 in them


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("cache", [False, True], ids=["nocache", "cache"])
@pytest.mark.parametrize("addc", [False, True], ids=["plain", "addc"])
def test_talk3_tea_is_three_tea_forwards(grid, cache, addc):
    m = _model()
    m.context_cache(cache)
    clip = _clip(grid, addc=addc)
    x, pos, neg, kw, aud, null, add = clip
    L, D = grid[0] * grid[1] * grid[2], CFG["dim"]
    new = lambda: torch.full((1, L, D), SENTINEL, dtype=torch.bfloat16, device="cuda")      # noqa: E731
    # the residuals a skip reads: left by an all-store step at another timestep (the negative buffer ends as drop-text's)
    P_old, N_old = new(), new()
    _three_tea_forwards(m, clip, (1, 1, 1), P_old, N_old, ts=TS_OLD)
    assert not (P_old == SENTINEL).all() and not (N_old == SENTINEL).all() and not torch.equal(P_old, N_old)
    m.stage_audio(0, aud)
    m.stage_audio(1, null)
    call = lambda modes, P, N, ts=TS: tuple(o.clone() for o in m.forward_talk3(      # noqa: E731
        x, ts, pos, neg, add_condition=add, tea_modes=modes, residual_cond=P, residual_uncond=N, residual_drop_text=N, **kw))
    # an all-store call leaves what the three forwards left
    P1, N1 = new(), new()
    got = call((1, 1, 1), P1, N1, TS_OLD)
    assert torch.equal(P1, P_old) and torch.equal(N1, N_old)
    plain = tuple(o.clone() for o in m.forward_talk3(x, TS, pos, neg, add_condition=add, **kw))
    for modes in TRIPLES:
        Pr, Nr, Pg, Ng = P_old.clone(), N_old.clone(), P_old.clone(), N_old.clone()
        _prefill(modes, Pr, Nr)
        _prefill(modes, Pg, Ng)
        want = _three_tea_forwards(m, clip, modes, Pr, Nr)
        got = call(modes, Pg, Ng)
        for name, g, w in zip(("cond", "uncond", "drop_text"), got, want):
            assert torch.equal(g, w), (modes, name, errs(g, w))
        assert torch.equal(Pg, Pr) and torch.equal(Ng, Nr), (modes, "residuals")
        if modes[0] == 1:
            assert not (Pg == SENTINEL).all()
        if 1 in modes[1:]:
            assert not torch.equal(Ng, N_old)
        if 1 not in modes:                       # nothing stores: the buffers are only read
            assert torch.equal(Pg, P_old) and torch.equal(Ng, N_old)
        if modes == (1, 1, 2):
            # drop-text read what uncond stored in THIS call, not the old residual
            m.set_audio(aud)
            from_old = m.forward(x, TS, neg, add_condition=add, tea_mode=2, residual=N_old.clone(), **kw)
            m.set_audio(None)
            assert not torch.equal(got[2], from_old)
        if modes == (1, 2, 1):
            # uncond read the old residual, not the one drop-text stored behind it
            m.set_audio(null)
            from_old = m.forward(x, TS, neg, tea_mode=2, residual=N_old.clone(), **kw).clone()
            from_new = m.forward(x, TS, neg, tea_mode=2, residual=Ng, **kw).clone()
            m.set_audio(None)
            assert torch.equal(got[1], from_old) and not torch.equal(got[1], from_new)
        if modes == (2, 2, 2):
            # uncond and drop-text skip from one buffer: equal rows without add_condition, different with it
            assert torch.equal(got[1], got[2]) == (not addc)
            assert not torch.equal(got[0], got[1])
        if 0 in modes:
            for k in range(3):
                if modes[k] == 0:
                    assert torch.equal(got[k], plain[k]), (modes, k)
    # all modes 0 through the new arguments is the plain call
    zero = m.forward_talk3(x, TS, pos, neg, add_condition=add, tea_modes=(0, 0, 0), **kw)
    assert all(torch.equal(z, p) for z, p in zip(zero, plain))
    # separate buffers for uncond and drop-text are served too: each keeps its own store
    Pg, Nu, Nd = new(), new(), new()
    m.forward_talk3(x, TS_OLD, pos, neg, add_condition=add, tea_modes=(1, 1, 1), residual_cond=Pg, residual_uncond=Nu, residual_drop_text=Nd, **kw)
    Nur = new()
    m.set_audio(null)
    m.forward(x, TS_OLD, neg, tea_mode=1, residual=Nur, **kw)
    m.set_audio(None)
    assert torch.equal(Pg, P_old) and torch.equal(Nd, N_old) and torch.equal(Nu, Nur) and not torch.equal(Nu, Nd)


# The skip kernel at a product width: the tiny talk model (dim 256) runs it with partly filled lanes only.  Dim 1536 is every lane full at three chunks; the
# three armed forwards it is held against run add_bf16 (+ add_bf16) + svi_launch_ln_mod, the multi-row kernel at this width.  15 rows: the last workgroup
# runs three.  The triples: every branch skips (three served rows, uncond without add_condition), cond and drop-text only, uncond and drop-text only.
WIDE_CFG = dict(CFG, dim=1536, ffn_dim=256, num_layers=1)


@pytest.mark.parametrize("addc", [False, True], ids=["plain", "addc"])
def test_talk3_tea_skip_at_a_product_width(addc):
    grid = (1, 3, 5)
    m = _model("wide", WIDE_CFG)
    m.context_cache(True)
    clip = _clip(grid, addc=addc, dim=WIDE_CFG["dim"])
    x, pos, neg, kw, aud, null, add = clip
    L, D = grid[0] * grid[1] * grid[2], WIDE_CFG["dim"]
    P_old, N_old = (torch.full((1, L, D), SENTINEL, dtype=torch.bfloat16, device="cuda") for _ in range(2))
    _three_tea_forwards(m, clip, (1, 1, 1), P_old, N_old, ts=TS_OLD)
    assert not (P_old == SENTINEL).all() and not (N_old == SENTINEL).all() and not torch.equal(P_old, N_old)
    m.stage_audio(0, aud)
    m.stage_audio(1, null)
    plain = tuple(o.clone() for o in m.forward_talk3(x, TS, pos, neg, add_condition=add, **kw))
    for modes in ((2, 2, 2), (2, 0, 2), (1, 2, 2)):
        Pr, Nr, Pg, Ng = P_old.clone(), N_old.clone(), P_old.clone(), N_old.clone()
        _prefill(modes, Pr, Nr)
        _prefill(modes, Pg, Ng)
        want = _three_tea_forwards(m, clip, modes, Pr, Nr)
        got = tuple(o.clone() for o in m.forward_talk3(x, TS, pos, neg, add_condition=add, tea_modes=modes, residual_cond=Pg, residual_uncond=Ng,
                                                       residual_drop_text=Ng, **kw))
        for name, g, w in zip(("cond", "uncond", "drop_text"), got, want):
            assert torch.equal(g, w), (modes, name, errs(g, w))
        assert torch.equal(Pg, Pr) and torch.equal(Ng, Nr), (modes, "residuals")
        assert torch.equal(Ng, N_old) and (torch.equal(Pg, P_old) == (modes[0] == 2))          # a skip reads its residual, a store replaces it
        if modes == (2, 2, 2):
            assert torch.equal(got[1], got[2]) == (not addc) and not torch.equal(got[0], got[1])
        for k in range(3):
            assert torch.equal(got[k], plain[k]) == (modes[k] != 2), (modes, k)                # a skipped branch is not a computed one
    m.context_cache(False)


def test_talk3_tea_refusals_leave_the_outputs_alone():
    from svi_hip import _lib as L
    m = _model()
    grid = synth.TALK_GRID
    x, pos, neg, kw, aud, null, add = _clip(grid)
    Lr, D = grid[0] * grid[1] * grid[2], CFG["dim"]
    n = Lr * D
    m.stage_audio(0, aud)
    m.stage_audio(1, null)
    outs = [torch.full_like(x, SENTINEL) for _ in range(3)]
    P = torch.zeros((1, Lr, D), dtype=torch.bfloat16, device="cuda")
    big = torch.zeros(2 * n, dtype=torch.bfloat16, device="cuda")
    N, N_shifted = big[:n].view(1, Lr, D), big[8:8 + n].view(1, Lr, D)
    # a residual that lies inside an output buffer
    wide = torch.full((n + x.numel(),), SENTINEL, dtype=torch.bfloat16, device="cuda")
    out_in_wide, res_in_wide = wide[:x.numel()].view(x.shape), wide[x.numel() - 8:x.numel() - 8 + n].view(1, Lr, D)
    # ... and one that lies inside the buffer the latents are in
    xwide = torch.zeros(x.numel() + n, dtype=torch.bfloat16, device="cuda")
    x_in_wide, res_in_xwide = xwide[:x.numel()].view(x.shape), xwide[x.numel() - 8:x.numel() - 8 + n].view(1, Lr, D)
    x_in_wide.copy_(x)

    def call(modes, rc, ru, rd, out_uncond=outs[1], x_=x):
        return m.forward_talk3(x_, TS, pos, neg, add_condition=add, tea_modes=modes, residual_cond=rc, residual_uncond=ru, residual_drop_text=rd,
                               out_cond=outs[0], out_uncond=out_uncond, out_drop_text=outs[2], **kw)
    with pytest.raises(RuntimeError, match="residual_uncond and residual_drop_text overlap without being the same buffer"):
        call((1, 1, 1), P, N, N_shifted)
    with pytest.raises(RuntimeError, match="residual_cond overlaps residual_drop_text"):
        call((2, 1, 2), N_shifted, P, N)
    with pytest.raises(RuntimeError, match="residual_cond overlaps residual_uncond"):
        call((1, 2, 0), N, N, None)
    with pytest.raises(RuntimeError, match="residual_drop_text overlaps out_uncond"):
        call((1, 1, 2), P, N, res_in_wide, out_uncond=out_in_wide)
    with pytest.raises(RuntimeError, match="residual_cond overlaps the input x"):
        call((1, 0, 0), res_in_xwide, None, None, x_=x_in_wide)
    with pytest.raises(RuntimeError, match=r"tea_uncond = 3"):
        call((1, 3, 1), P, N, N)
    with pytest.raises(ValueError, match="needs residual_drop_text"):
        call((0, 0, 2), None, None, None)
    # the library itself names a missing residual; the slots are asked for even when every branch skips
    ts = TS.cuda()
    _, _, T, H, W = x.shape
    st = L.lib().svi_dit_forward_talk3_tea(m._h, L.ptr(x), L.ptr(ts), L.ptr(pos), L.ptr(neg), L.ptr(kw["clip_feature"]), L.ptr(kw["y"]), L.ptr(add),
                                           L.ptr(outs[0]), L.ptr(outs[1]), L.ptr(outs[2]), T, H, W, pos.shape[1], 1, 2, 2, L.ptr(P), None, L.ptr(N),
                                           L.current_stream())
    assert st != 0 and "tea_uncond = 2 needs residual_uncond" in L.last_error()
    m.stage_audio(1, None)
    with pytest.raises(RuntimeError, match="slot 1 is not staged"):
        call((2, 2, 2), P, N, N)
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in outs) and bool((wide == SENTINEL).all())


# ---- the loop ----------------------------------------------------------------------------------------------------------------------
class Scripted:
    """A TeaCache stand-in whose check() answers from a fixed list (True = skip) and records what it answered; the attributes are the ones
    model_fn_wan_video and the loop touch."""

    def __init__(self, answers):
        self.answers, self.log = list(answers), []
        self.previous_residual = self.previous_hidden_states = None

    def check(self, dit, x, t_mod):
        skip = self.answers[len(self.log)]
        self.log.append(skip)
        return skip


# eleven steps: every triple a positive and a negative cache can produce, the all-skip and the all-store step again after more than TALK_TEA_GRAPHS others
SCHEDULE = [(1, 1, 1), (2, 2, 2), (1, 1, 2), (2, 2, 1), (1, 2, 2), (2, 1, 1), (1, 2, 1), (2, 1, 2), (2, 2, 2), (1, 1, 1), (1, 1, 1)]


def _scripted_pair():
    return Scripted([t[0] == 2 for t in SCHEDULE]), Scripted([m == 2 for t in SCHEDULE for m in t[1:]])


def _recorded(P, N):
    return [(2 if p else 1, 2 if N.log[2 * i] else 1, 2 if N.log[2 * i + 1] else 1) for i, p in enumerate(P.log)]


def _sampler_inputs(k=0):
    import svi_hip
    f, h, w = synth.TALK_GRID
    x, pos, neg, kw, aud, null, add = _clip(synth.TALK_GRID, k=k)
    lat = dev(svi_hip.generate_noise((1, 16, f, 2 * h, 2 * w), seed=31 + k, device="cpu", dtype=torch.float32))
    return lat, pos, neg, kw, aud, null, add


@pytest.fixture
def step_latents(monkeypatch):
    """Records the latents after every three-way guidance + Euler update (ops.cfg3_step_, which every talk loop ends its step with)."""
    import svi_hip
    seen = []
    orig = svi_hip.ops.cfg3_step_

    def spy(latents, *a, **k):
        r = orig(latents, *a, **k)
        seen.append(latents.clone())
        return r
    monkeypatch.setattr(svi_hip.ops, "cfg3_step_", spy)
    return seen


@pytest.mark.parametrize("addc", [False, True], ids=["plain", "addc"])
def test_scripted_schedule_graphed_is_eager_is_by_hand(addc, step_latents):
    import svi_hip
    from svi_hip.pipeline import TALK_TEA_GRAPHS
    m = _model()
    lat, pos, neg, kw, aud, null, add = _sampler_inputs()
    add = add if addc else None
    n = len(SCHEDULE)
    steps = dict(num_inference_steps=n, text_scale=5.0, audio_scale=4.0)

    def run(loop):
        P, N = _scripted_pair()
        del step_latents[:]
        out = loop.sample_multitalk(lat, pos, neg, aud, null, add_condition=add, tea_cache_posi=P, tea_cache_nega=N, **steps, **kw)
        return out, [s.clone() for s in step_latents], P, N
    eager_loop, fast_loop = svi_hip.DenoiseLoop(m, graph=False), svi_hip.DenoiseLoop(m, graph=True)
    want, want_steps, P, N = run(eager_loop)
    # the schedule, from what the eager run's caches answered: all eight triples, more distinct ones than graphs are kept
    assert _recorded(P, N) == SCHEDULE and len(want_steps) == n
    assert set(SCHEDULE) == set(itertools.product((1, 2), repeat=3)) and len(set(SCHEDULE)) > TALK_TEA_GRAPHS
    got, got_steps, Pg, Ng = run(fast_loop)
    assert _recorded(Pg, Ng) == SCHEDULE
    for i, (g, w) in enumerate(zip(got_steps, want_steps)):
        assert torch.equal(g, w), (i, SCHEDULE[i], errs(g, w))
    assert torch.equal(got, want) and len(got_steps) == n
    assert torch.equal(Pg.previous_residual, P.previous_residual) and torch.equal(Ng.previous_residual, N.previous_residual)
    counts = {t: SCHEDULE.count(t) for t in set(SCHEDULE)}
    assert fast_loop.talk_tea_counts == counts and fast_loop.tea_counts == {"computed": sum(t[0] == 1 for t in SCHEDULE), "skipped": sum(t[0] == 2 for t in SCHEDULE)}
    # eight first captures, then (2, 2, 2) and (1, 1, 1) again after four others evicted them; the last step replays
    assert eager_loop.captures == 0 and fast_loop.captures == 10
    assert not fast_loop._tea_graphs and not m._audio_slots and not m._ctx_cache_on
    # by hand: three model_fn_wan_talk_video calls per step with the cache objects, then the fused guidance + Euler update
    P, N = _scripted_pair()
    sch = svi_hip.FlowMatchScheduler(shift=5, sigma_min=0.0, extra_one_step=True)
    sch.set_timesteps(n, shift=5.0)
    x = lat.clone()
    fn = svi_hip.model_fn_wan_talk_video
    m.context_cache(True)
    try:
        for i, t in enumerate(sch.timesteps):
            tt = t.reshape(1).to(device="cuda", dtype=torch.float32)
            c = fn(m, x, tt, pos, add_condition=add, audio_embed_tuple=aud, tea_cache=P, **kw)
            u = fn(m, x, tt, neg, audio_embed_tuple=null, tea_cache=N, **kw)
            d = fn(m, x, tt, neg, add_condition=add, audio_embed_tuple=aud, tea_cache=N, **kw)
            svi_hip.ops.cfg3_step_(x, c, u, d, 5.0, 4.0, sch.step_delta(t))
            assert torch.equal(x, got_steps[i]), (i, SCHEDULE[i], errs(x, got_steps[i]))
    finally:
        m.context_cache(False)
    assert _recorded(P, N) == SCHEDULE


def test_graph_bound_holds_during_a_clip():
    import svi_hip
    from svi_hip.pipeline import TALK_TEA_GRAPHS
    m = _model()
    lat, pos, neg, kw, aud, null, add = _sampler_inputs()
    loop = svi_hip.DenoiseLoop(m, graph=True)
    P, N = _scripted_pair()
    most = []
    bar = lambda it: (most.append(len(loop._tea_graphs)) or t for t in it)      # noqa: E731
    loop.sample_multitalk(lat, pos, neg, aud, null, add_condition=add, tea_cache_posi=P, tea_cache_nega=N, num_inference_steps=len(SCHEDULE),
                          text_scale=5.0, audio_scale=4.0, progress_bar_cmd=bar, **kw)
    assert max(most) == TALK_TEA_GRAPHS and len(most) == len(SCHEDULE)


class Recording:
    """svi_hip.TeaCache with a record of its answers."""

    def __new__(cls, *a):
        import svi_hip

        class _R(svi_hip.TeaCache):
            def __init__(self, *args):
                super().__init__(*args)
                self.log = []

            def check(self, dit, x, t_mod):
                skip = super().check(dit, x, t_mod)
                self.log.append(skip)
                return skip
        return _R(*a)


def _same_state(a, b):
    return (a.step == b.step and a.accumulated_rel_l1_distance == b.accumulated_rel_l1_distance and a.log == b.log
            and torch.equal(a.previous_modulated_input, b.previous_modulated_input) and torch.equal(a.previous_residual, b.previous_residual))


@pytest.mark.parametrize("addc", [False, True], ids=["plain", "addc"])
def test_real_teacache_graphed_is_eager(addc):
    import svi_hip
    m = _model()
    lat, pos, neg, kw, aud, null, add = _sampler_inputs()
    add = add if addc else None

    def run(loop):
        P, N = Recording(TEA_STEPS, TEA_THRESH_MIXED, TEA_MODEL), Recording(TEA_STEPS, TEA_THRESH_MIXED, TEA_MODEL)
        out = loop.sample_multitalk(lat, pos, neg, aud, null, add_condition=add, tea_cache_posi=P, tea_cache_nega=N, num_inference_steps=TEA_STEPS,
                                    text_scale=5.0, audio_scale=4.0, **kw)
        return out, P, N
    want, P, N = run(svi_hip.DenoiseLoop(m, graph=False))
    print("eager decisions:", _recorded(P, N))
    # both kinds of step for both objects, from the eager run itself (the first answers are forced: look behind them)
    assert len(P.log) == TEA_STEPS and len(N.log) == 2 * TEA_STEPS
    forced = (0, TEA_STEPS - 1, TEA_STEPS, 2 * TEA_STEPS - 1)          # the calls of a cache that always compute (its step counter wraps at num_inference_steps)
    assert True in P.log and False in P.log[1:-1] and True in N.log and any(not s for i, s in enumerate(N.log) if i not in forced)
    fast = svi_hip.DenoiseLoop(m)                   # graph=None: the default is the graphed path
    got, Pg, Ng = run(fast)
    assert torch.equal(got, want), errs(got, want)
    assert _same_state(Pg, P) and _same_state(Ng, N)
    assert fast.captures >= len(set(_recorded(P, N))) and sum(fast.talk_tea_counts.values()) == TEA_STEPS
    assert fast.talk_tea_counts == {t: _recorded(P, N).count(t) for t in set(_recorded(P, N))}
    # the threshold form builds the two objects itself
    again = svi_hip.DenoiseLoop(m).sample_multitalk(lat, pos, neg, aud, null, add_condition=add, tea_cache_l1_thresh=TEA_THRESH_MIXED,
                                                    tea_cache_model_id=TEA_MODEL, num_inference_steps=TEA_STEPS, text_scale=5.0, audio_scale=4.0, **kw)
    assert torch.equal(again, want)
    # one side without an object: its modes are 0
    P1 = Recording(TEA_STEPS, TEA_THRESH_MIXED, TEA_MODEL)
    want1 = svi_hip.DenoiseLoop(m, graph=False).sample_multitalk(lat, pos, neg, aud, null, add_condition=add, tea_cache_posi=P1, num_inference_steps=TEA_STEPS,
                                                                 text_scale=5.0, audio_scale=4.0, **kw)
    loop1 = svi_hip.DenoiseLoop(m, graph=True)
    got1 = loop1.sample_multitalk(lat, pos, neg, aud, null, add_condition=add, tea_cache_posi=Recording(TEA_STEPS, TEA_THRESH_MIXED, TEA_MODEL),
                                  num_inference_steps=TEA_STEPS, text_scale=5.0, audio_scale=4.0, **kw)
    assert torch.equal(got1, want1) and set(loop1.talk_tea_counts) == {(1, 0, 0), (2, 0, 0)}


def test_resident_loop_replays_teacache_clips():
    """Two clips of one shape with different inputs on ONE resident loop, TeaCache on: the second clip captures nothing — the residuals are slots, so
    every triple's graph still holds — and equals a fresh loop that is not resident."""
    import svi_hip
    from svi_hip.pipeline import TALK_TEA_GRAPHS
    m, ref = _model("a"), _model("b")
    loop = svi_hip.DenoiseLoop(m, graph=True, resident=True)
    tea = dict(tea_cache_l1_thresh=TEA_THRESH_FOUR, tea_cache_model_id=TEA_MODEL, num_inference_steps=TEA_STEPS, text_scale=5.0, audio_scale=4.0)
    try:
        outs = []
        for k in range(2):
            lat, pos, neg, kw, aud, null, add = _sampler_inputs(k)
            want = svi_hip.DenoiseLoop(ref, graph=True).sample_multitalk(lat, pos, neg, aud, null, add_condition=add, **tea, **kw)
            got = loop.sample_multitalk(lat, pos, neg, aud, null, add_condition=add, **tea, **kw)
            assert torch.equal(got, want), (k, errs(got, want))
            outs.append(got)
            if k == 0:
                caps, graphs = loop.captures, {s: g["graph"] for s, g in loop._tea_graphs.items()}
                counts = dict(loop.talk_tea_counts)
                assert 2 <= len(counts) <= TALK_TEA_GRAPHS and caps == len(counts) and 2 in {t[0] for t in counts} and 1 in {t[0] for t in counts}
            else:
                assert loop.captures == caps and loop.talk_tea_counts == counts
                assert {s: g["graph"] for s, g in loop._tea_graphs.items()} == graphs          # the very graph objects
        assert not torch.equal(outs[0], outs[1])
    finally:
        loop.close()
    assert not m._audio_slots and not m._ctx_cache_on


# ---- install() -----------------------------------------------------------------------------------------------------------------------
# tests/test_gpu_talk3.py's stand-in for the talk pipeline's module, in a copy of its own: the reference's parameter list, its three calls per step with
# the TeaCache dicts spread into them, its guidance arithmetic on bf16 tensors.
TALK_SAMPLER_SRC = '''
def model_fn_wan_talk_video(dit, x, timestep, context, **kwargs):
    raise AssertionError("the PyTorch model_fn was called: install() did not take effect")


class SVITalkVideoPipeline:
    def __init__(self, dit, scheduler):
        self.dit, self.vae, self.scheduler, self.device, self.python_loops = dit, None, scheduler, "cuda", 0

    def _sample_with_multitalk(self, latents, prompt_emb_posi, prompt_emb_nega, image_emb, extra_input, tea_cache_posi, tea_cache_nega, usp_kwargs, condition, audio_embed_tuple, audio_embed_tuple_null, use_controlnet, cfg_scale, progress_bar_cmd):
        self.python_loops += 1
        shared = dict(**image_emb, **extra_input, **usp_kwargs, use_controlnet=use_controlnet)
        for i, t in enumerate(progress_bar_cmd(self.scheduler.timesteps)):
            t = t.unsqueeze(0).to(device=self.device)
            cond = model_fn_wan_talk_video(self.dit, latents, timestep=t, **prompt_emb_posi, **tea_cache_posi, add_condition=condition, audio_embed_tuple=audio_embed_tuple, **shared)
            if cfg_scale["text"] != 1.0 or cfg_scale["audio"] != 1.0:
                uncond = model_fn_wan_talk_video(self.dit, latents, timestep=t, **prompt_emb_nega, **tea_cache_nega, audio_embed_tuple=audio_embed_tuple_null, **shared)
                drop = model_fn_wan_talk_video(self.dit, latents, timestep=t, **prompt_emb_nega, **tea_cache_nega, add_condition=condition, audio_embed_tuple=audio_embed_tuple, **shared)
                pred = uncond + cfg_scale["text"] * (cond - drop) + cfg_scale["audio"] * (drop - uncond)
            else:
                pred = cond
            latents = self.scheduler.step(pred, self.scheduler.timesteps[i], latents)
        return latents
'''


def test_install_serves_clips_with_teacache_objects():
    import svi_hip
    from test_gpu_install import wan_model_double
    modname = "svi_video_talk_tea_double"
    mod = types.ModuleType(modname)
    sys.modules[modname] = mod
    try:
        exec(compile(TALK_SAMPLER_SRC, modname + ".py", "exec"), mod.__dict__)
        mod.SVITalkVideoPipeline.__module__ = modname
        dits = [wan_model_double(CFG, SEED)[0] for _ in range(2)]
        for d in dits:
            d.enable_multitalk = True
        sch = svi_hip.FlowMatchScheduler(shift=5, sigma_min=0.0, extra_one_step=True)
        sch.set_timesteps(TEA_STEPS, shift=5.0)
        slow_pipe, fast_pipe = mod.SVITalkVideoPipeline(dits[0], sch), mod.SVITalkVideoPipeline(dits[1], sch)
        svi_hip.install(slow_pipe, vae=False, sampler=False)
        svi_hip.install(fast_pipe, vae=False)
        loop = fast_pipe._svi_hip_loop

        def args(k, **over):
            x, pos, neg, kw, aud, null, add = _clip(synth.TALK_GRID, k=k)
            P, N = Recording(TEA_STEPS, TEA_THRESH_MIXED, TEA_MODEL), Recording(TEA_STEPS, TEA_THRESH_MIXED, TEA_MODEL)
            a = dict(latents=x, prompt_emb_posi={"context": pos}, prompt_emb_nega={"context": neg}, image_emb=kw, extra_input={},
                     tea_cache_posi={"tea_cache": P}, tea_cache_nega={"tea_cache": N}, usp_kwargs={}, condition=add, audio_embed_tuple=aud,
                     audio_embed_tuple_null=null, use_controlnet=False, cfg_scale={"text": 5.0, "audio": 4.0}, progress_bar_cmd=lambda it: it)
            a.update(over)
            return tuple(a.values()), P, N
        for k in range(2):
            a, P, N = args(k)
            want = slow_pipe._sample_with_multitalk(*a)
            b, Pg, Ng = args(k)
            got = fast_pipe._sample_with_multitalk(*b)
            assert got.dtype == torch.bfloat16 and torch.equal(got, want), (k, errs(got, want))
            # the pipeline's own objects were driven, and end as its own loop leaves them
            assert False in P.log[1:-1] and True in P.log and _same_state(Pg, P) and _same_state(Ng, N)
            assert Pg.previous_residual is not Ng.previous_residual
        assert slow_pipe.python_loops == 2 and fast_pipe.python_loops == 0            # the original sampler was not called
        assert set(loop.talk_tea_counts) == set(_recorded(P, N))
        # anything else that asks for the pipeline's loop still gets it, TeaCache objects or not
        a, P, N = args(0, extra_input={"unused": 1})
        b, _, _ = args(0, extra_input={"unused": 1})
        assert torch.equal(fast_pipe._sample_with_multitalk(*b), slow_pipe._sample_with_multitalk(*a)) and fast_pipe.python_loops == 1
        loop.close()
    finally:
        del sys.modules[modname]
