"""-m gpu: the talk step as one call — svi_dit_audio_slot + svi_dit_forward_talk3 (WanDiT.stage_audio / forward_talk3), the graphed and resident
DenoiseLoop.sample_multitalk on top of it, and install()'s `_hip_sample_with_multitalk`.

Everything is compared bit for bit (torch.equal), within one process, against what the call replaces: three model_fn_wan_talk_video calls per step
(conditional: prompt, audio, add_condition; unconditional: negative prompt, null audio; drop-text: negative prompt, audio, add_condition).  The one-call
form runs the same kernels on the same operands — it only stops repeating what the three forwards share — so there is no tolerance to state.  The
sampler additionally stays within the existing 5e-2 of the reference's own _sample_with_multitalk (golden/dit_tiny_talk.npz)."""
import sys
import types

import pytest
import torch

import synth
from gpu_util import dev, errs

pytestmark = pytest.mark.gpu

CFG, SEED = synth.TINY_DIT_TALK, synth.TALK_SEED
GRIDS = [synth.TALK_GRID, (1, 4, 6), (3, 3, 5)]      # the talk golden's grid; one frame (n_latter = 0, audio_latter NULL); 45 tokens (no multiple of 8)
TS = torch.tensor([637.5])
_MODELS = {}


def _model(key="a"):
    """One WanDiT per key for the whole module (same weights: instances give the same bits); every test starts with the cache off, nothing armed,
    no slot staged."""
    import svi_hip
    m = _MODELS.get(key)
    if m is None:
        sd = {k: torch.from_numpy(v) for k, v in synth.dit_state_dict(SEED, **CFG).items()}
        m = _MODELS[key] = svi_hip.WanDiT.from_state_dict(sd, eps=1e-6, num_heads=synth.num_heads_of(CFG), **CFG)
    m.context_cache(False)
    m.set_audio(None)
    m.stage_audio(0, None)
    m.stage_audio(1, None)
    return m


def _clip(grid, k=0, addc=True):
    """One clip's inputs on the device (bf16): latents, the two prompts, clip_feature / y, the audio tuple, the null audio tuple, add_condition."""
    f, h, w = grid
    s = SEED + 100 * k
    x = dev(synth.randn(s + 1, 1, 16, f, 2 * h, 2 * w))
    pos = dev(synth.text_context(s + 2, 20, CFG["text_dim"], 13))
    neg = dev(synth.text_context(s + 12, 20, CFG["text_dim"], 4))
    kw = dict(clip_feature=dev(synth.randn(s + 3, 1, 257, 1280)), y=dev(synth.randn(s + 4, 1, 20, f, 2 * h, 2 * w)))
    aud = tuple(dev(a) for a in synth.audio_windows(s + 5, f))
    null = tuple(dev(a) for a in synth.audio_windows(s + 7, f))
    add = dev(0.5 * synth.randn(s + 9, 1, f * h * w, CFG["dim"])) if addc else None
    return x, pos, neg, kw, aud, null, add


def _three_forwards(m, x, pos, neg, kw, aud, null, add, ts=TS):
    import svi_hip
    fn = svi_hip.model_fn_wan_talk_video
    c = fn(m, x, ts, pos, add_condition=add, audio_embed_tuple=aud, **kw)
    u = fn(m, x, ts, neg, audio_embed_tuple=null, **kw)
    d = fn(m, x, ts, neg, add_condition=add, audio_embed_tuple=aud, **kw)
    return c, u, d


def _talk3(m, x, pos, neg, kw, aud, null, add, ts=TS, stage=True, **outs):
    if stage:
        m.stage_audio(0, aud)
        m.stage_audio(1, null)
    return m.forward_talk3(x, ts, pos, neg, add_condition=add, **outs, **kw)


def _same(got, want):
    return all(torch.equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("cache", [False, True], ids=["nocache", "cache"])
@pytest.mark.parametrize("addc", [False, True], ids=["plain", "addc"])
def test_forward_talk3_is_three_talk_forwards(grid, cache, addc):
    m = _model()
    m.context_cache(cache)
    clip = _clip(grid, addc=addc)
    want = _three_forwards(m, *clip)
    got = _talk3(m, *clip)
    assert all(g.shape == clip[0].shape and g.dtype == torch.bfloat16 for g in got)
    for name, g, w in zip(("cond", "uncond", "drop_text"), got, want):
        assert torch.equal(g, w), (name, errs(g, w))
    # each branch really read its own prompt / audio: drop-text shares the prompt with uncond and the audio with cond, and equals neither
    assert not torch.equal(got[2], got[0]) and not torch.equal(got[2], got[1])
    assert _same(_talk3(m, *clip, stage=False), want)          # and again, on the staged slots (cache on: on the cached prompts)


def test_slots_own_their_data_and_restage_in_place():
    m = _model()
    m.context_cache(True)
    grid = synth.TALK_GRID
    x, pos, neg, kw, aud, null, add = _clip(grid)
    first = _talk3(m, x, pos, neg, kw, aud, null, add)
    other = _clip(grid, k=1)
    aud_b, null_b = other[4], other[5]
    keep = tuple(a.clone() for a in aud), tuple(a.clone() for a in null)
    for dst, src in zip(aud + null, aud_b + null_b):            # the caller's tensors now hold another clip's audio
        dst.copy_(src)
    assert _same(_talk3(m, x, pos, neg, kw, None, None, add, stage=False), first)
    # the clip boundary: the same frame count staged again — nothing moves, the results are the new audio's
    gen = m.generation()
    m.stage_audio(0, aud_b)
    m.stage_audio(1, null_b)
    assert m.generation() == gen
    got = m.forward_talk3(x, TS, pos, neg, add_condition=add, **kw)
    assert m.generation() == gen
    assert _same(got, _three_forwards(m, x, pos, neg, kw, aud_b, null_b, add)) and not torch.equal(got[0], first[0])
    m.stage_audio(0, keep[0])
    m.stage_audio(1, keep[1])
    assert _same(m.forward_talk3(x, TS, pos, neg, add_condition=add, **kw), first)
    # another frame count, and freeing a slot, move the generation
    gen = m.generation()
    m.stage_audio(1, tuple(dev(a) for a in synth.audio_windows(5, 2)))
    g2 = m.generation()
    assert g2 != gen
    m.stage_audio(1, None)
    assert m.generation() != g2


def test_refusals_name_their_cause():
    import svi_hip
    from svi_hip import _lib as L
    m = _model()
    grid = synth.TALK_GRID
    x, pos, neg, kw, aud, null, add = _clip(grid)
    call = lambda **k: m.forward_talk3(x, TS, pos, neg, add_condition=add, **kw, **k)      # noqa: E731
    with pytest.raises(RuntimeError, match="slot 0 is not staged"):
        call()
    m.stage_audio(0, aud)
    with pytest.raises(RuntimeError, match="slot 1 is not staged"):
        call()
    short = tuple(dev(a) for a in synth.audio_windows(5, 2))
    m.stage_audio(1, short)
    with pytest.raises(RuntimeError, match="slot 1 covers 2 latent frames, the latents have 3"):
        call()
    m.stage_audio(1, null)
    m.set_audio(aud)
    with pytest.raises(RuntimeError, match="armed through svi_dit_set_audio"):
        call()
    m.set_audio(None)
    o = torch.empty_like(x)
    with pytest.raises(RuntimeError, match="aliased outputs"):
        call(out_cond=o, out_drop_text=o)
    two = torch.empty((2,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    with pytest.raises(RuntimeError, match="aliased outputs"):      # overlapping, not equal
        call(out_cond=two[:1], out_uncond=two.view(-1)[8:8 + x.numel()].view(x.shape))
    # the C entry points themselves: null outputs, a size the patch does not divide, a slot that does not exist
    lib, ts = L.lib(), TS.cuda()
    _, _, T, H, W = x.shape
    args = lambda oc, H_: (m._h, L.ptr(x), L.ptr(ts), L.ptr(pos), L.ptr(neg), L.ptr(kw["clip_feature"]), L.ptr(kw["y"]), L.ptr(add),      # noqa: E731
                           oc, L.ptr(o), L.ptr(two), T, H_, W, pos.shape[1], L.current_stream())
    assert lib.svi_dit_forward_talk3(*args(None, H)) != 0 and "null output" in L.last_error()
    assert lib.svi_dit_forward_talk3(*args(L.ptr(torch.empty_like(x)), H - 1)) != 0 and "not divisible by the patch size" in L.last_error()
    assert lib.svi_dit_audio_slot(m._h, 2, L.ptr(aud[0]), L.ptr(aud[1]), 2, L.current_stream()) != 0 and "slot 2" in L.last_error()
    assert lib.svi_dit_audio_slot(m._h, 0, L.ptr(aud[0]), None, 2, L.current_stream()) != 0 and "no audio_latter" in L.last_error()
    # a model without the audio modules
    c0 = synth.TINY_DIT
    plain = svi_hip.WanDiT.from_state_dict({k: torch.from_numpy(v) for k, v in synth.dit_state_dict(100, **c0).items()}, eps=1e-6,
                                           num_heads=synth.num_heads_of(c0), **c0)
    with pytest.raises(ValueError, match="without enable_multitalk"):
        plain.stage_audio(0, aud)
    assert lib.svi_dit_audio_slot(plain._h, 0, L.ptr(aud[0]), L.ptr(aud[1]), 2, L.current_stream()) != 0 and "without enable_multitalk" in L.last_error()
    ctx0 = dev(synth.text_context(3, 20, c0["text_dim"], 13))
    with pytest.raises(RuntimeError, match="without enable_multitalk"):
        plain.forward_talk3(x, TS, ctx0, ctx0.clone())
    # the Python side's shape checks
    with pytest.raises(ValueError, match="slot must be 0"):
        m.stage_audio(2, aud)
    with pytest.raises(ValueError, match="audio_embed_tuple must be"):
        m.stage_audio(0, (aud[0][:, :, :4], aud[1]))
    with pytest.raises(ValueError, match="same shape"):
        m.forward_talk3(x, TS, pos, neg[:, :10].contiguous(), add_condition=add, **kw)
    with pytest.raises(ValueError, match="one sample per forward"):
        m.forward_talk3(torch.cat([x, x]), TS, torch.cat([pos, pos]), torch.cat([neg, neg]), clip_feature=torch.cat([kw["clip_feature"]] * 2),
                        y=torch.cat([kw["y"]] * 2))
    with pytest.raises(ValueError, match="out_uncond must be"):
        call(out_uncond=torch.empty_like(x)[:, :8])
    with pytest.raises(ValueError, match="not divisible by the patch size"):
        m.forward_talk3(x[..., :-1], TS, pos, neg, add_condition=add, clip_feature=kw["clip_feature"], y=kw["y"][..., :-1])
    with pytest.raises(ValueError, match="add_condition must be"):
        m.forward_talk3(x, TS, pos, neg, add_condition=add[:, :-1], **kw)
    # none of it left anything behind: the valid call right after gives the three forwards' bits
    assert _same(call(), _three_forwards(m, x, pos, neg, kw, aud, null, add))


def _sampler_inputs():
    import svi_hip
    f, h, w = synth.TALK_GRID
    x, pos, neg, kw, aud, null, add = _clip(synth.TALK_GRID)
    lat = dev(svi_hip.generate_noise((1, 16, f, 2 * h, 2 * w), seed=31, device="cpu", dtype=torch.float32))
    return lat, pos, neg, kw, aud, null, add


@pytest.mark.parametrize("addc", [False, True], ids=["plain", "addc"])
def test_graphed_loop_is_the_eager_loop(golden, addc):
    """The inputs of tests/test_gpu_talk.py's sampler test (the golden's), 3 steps: the graphed one-call loop gives the eager three-call loop's bits
    with ONE capture, and both stay within the 5e-2 the eager loop is held to against the reference's sampler."""
    import svi_hip
    m = _model()
    lat, pos, neg, kw, aud, null, add = _sampler_inputs()
    extra = dict(add_condition=add) if addc else {}
    run = lambda loop: loop.sample_multitalk(lat, pos, neg, aud, null, num_inference_steps=3, text_scale=5.0, audio_scale=4.0, **extra, **kw)      # noqa: E731
    slow_loop, fast_loop = svi_hip.DenoiseLoop(m, graph=False), svi_hip.DenoiseLoop(m, graph=True)
    slow = run(slow_loop)
    fast = run(fast_loop)
    assert slow_loop.captures == 0 and fast_loop.captures == 1
    assert torch.equal(fast, slow), errs(fast, slow)
    assert not m._audio_slots and not m._ctx_cache_on            # a loop that is not resident leaves nothing behind
    default = svi_hip.DenoiseLoop(m)                             # graph=None: the single-rank loop's default is the graphed path
    assert torch.equal(run(default), slow) and default.captures == 1
    if not addc:
        g = golden("dit_tiny_talk.npz")
        r_fast, r_slow = errs(fast, g["sampler_latents"])[0], errs(slow, g["sampler_latents"])[0]
        print(f"talk sampler vs the reference's: graphed {r_fast:.3e}, eager {r_slow:.3e}")
        assert r_fast < 5e-2 and r_slow < 5e-2, (r_fast, r_slow)


def test_resident_loop_replays_across_clips():
    """Two clips of equal shapes with different latents, prompts, audio, null audio, conditioning on ONE resident loop: each equals a fresh eager loop on
    that clip's inputs, and the second clip replays the first clip's graph (the audio went to the slots in place).  Another frame count captures again."""
    import svi_hip
    m, ref = _model("a"), _model("b")              # the eager loops toggle their model's context cache: they get a model of their own
    loop = svi_hip.DenoiseLoop(m, graph=True, resident=True)
    steps = dict(num_inference_steps=3, text_scale=5.0, audio_scale=4.0)
    try:
        for k, grid, caps in ((0, synth.TALK_GRID, 1), (1, synth.TALK_GRID, 1), (2, (2, 4, 6), 2)):
            x, pos, neg, kw, aud, null, add = _clip(grid, k=k)
            want = svi_hip.DenoiseLoop(ref, graph=False).sample_multitalk(x, pos, neg, aud, null, add_condition=add, **steps, **kw)
            got = loop.sample_multitalk(x, pos, neg, aud, null, add_condition=add, **steps, **kw)
            assert torch.equal(got, want), (k, errs(got, want))
            assert loop.captures == caps, (k, loop.captures)
            if k == 1:
                assert not torch.equal(got, first)
            first = got
    finally:
        loop.close()
    assert not m._audio_slots and not m._ctx_cache_on


# A stand-in for the talk pipeline's module, as tests/test_gpu_install.py builds its stand-ins: a module-level `model_fn_wan_talk_video` that the sampler
# looks up through the module globals at call time, and a class whose `_sample_with_multitalk` has the reference's parameter list
# (tests/test_talk3_host.py compares install()'s sampler with the reference's own source where that exists) and makes the reference's three calls per
# step and its guidance arithmetic on bf16 tensors.
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


def test_install_binds_the_talk_sampler():
    import svi_hip
    from test_gpu_install import wan_model_double
    modname = "svi_video_talk_double"
    mod = types.ModuleType(modname)
    sys.modules[modname] = mod
    try:
        exec(compile(TALK_SAMPLER_SRC, modname + ".py", "exec"), mod.__dict__)
        mod.SVITalkVideoPipeline.__module__ = modname
        dits = [wan_model_double(CFG, SEED)[0] for _ in range(2)]        # the same weights twice: install() keys its handle by the module, one per pipeline
        for d in dits:
            d.enable_multitalk = True
        sch = svi_hip.FlowMatchScheduler(shift=5, sigma_min=0.0, extra_one_step=True)
        sch.set_timesteps(3, shift=5.0)
        slow_pipe, off_pipe, fast_pipe = mod.SVITalkVideoPipeline(dits[0], sch), mod.SVITalkVideoPipeline(dits[0], sch), mod.SVITalkVideoPipeline(dits[1], sch)
        svi_hip.install(slow_pipe, vae=False, sampler=False)
        svi_hip.install(off_pipe, vae=False, sampler=False)
        svi_hip.install(fast_pipe, vae=False)
        assert "_sample_with_multitalk" not in off_pipe.__dict__                       # install(sampler=False) leaves the sampler alone
        assert fast_pipe._sample_with_multitalk.__func__ is svi_hip.pipeline._hip_sample_with_multitalk
        assert fast_pipe._svi_hip_original_talk_sampler.__func__ is mod.SVITalkVideoPipeline._sample_with_multitalk
        assert type(fast_pipe) is mod.SVITalkVideoPipeline                             # (not taken for a pipeline whose loop is inline in __call__)
        loop = fast_pipe._svi_hip_loop
        assert loop.resident

        def args(k, scales=(5.0, 4.0), latents=None, **over):
            x, pos, neg, kw, aud, null, add = _clip(synth.TALK_GRID, k=k)
            a = dict(latents=x if latents is None else latents, prompt_emb_posi={"context": pos}, prompt_emb_nega={"context": neg}, image_emb=kw, extra_input={},
                     tea_cache_posi={"tea_cache": None}, tea_cache_nega={"tea_cache": None}, usp_kwargs={}, condition=add, audio_embed_tuple=aud,
                     audio_embed_tuple_null=null, use_controlnet=False, cfg_scale={"text": scales[0], "audio": scales[1]}, progress_bar_cmd=lambda it: it)
            a.update(over)
            return tuple(a.values())
        wants = [slow_pipe._sample_with_multitalk(*args(k)) for k in range(2)]
        assert slow_pipe.python_loops == 2
        for k in range(2):
            a = args(k)
            before = a[0].clone()
            got = fast_pipe._sample_with_multitalk(*a)
            assert torch.equal(a[0], before)                                           # the caller's latents are left alone
            assert got.dtype == torch.bfloat16 and torch.equal(got, wants[k]), (k, errs(got, wants[k]))
        assert fast_pipe.python_loops == 0 and loop.captures == 1                      # the second clip replayed the first clip's step
        # what the fast loop does not cover reaches the pipeline's own sampler, over the swapped model function
        n = 0
        for over in (dict(scales=(1.0, 1.0)), dict(latents=_clip(synth.TALK_GRID)[0].float()), dict(extra_input={"unused": 1})):
            a = args(0, **over)
            got, want = fast_pipe._sample_with_multitalk(*a), slow_pipe._sample_with_multitalk(*a)
            n += 1
            assert fast_pipe.python_loops == n and torch.equal(got.float(), want.float())
        with pytest.raises(NotImplementedError, match="controlnet"):
            fast_pipe._sample_with_multitalk(*args(0, use_controlnet=True))
        assert fast_pipe.python_loops == n + 1
        loop.close()
    finally:
        del sys.modules[modname]
