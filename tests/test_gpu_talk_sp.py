"""-m gpu: the talk variant on sequence-parallel shards.

The audio cross-attention is a block-diagonal attention over frames (models/attention.py:318-371): a frame's h*w rows attend to that frame's 32
audio tokens.  A shard's rows start and end anywhere inside frames, so it runs as ONE frame-segmented launch (svi_attention_frames_fwd), held
here to the per-frame launches it replaces bit for bit and to fp64 attention.  Every rank projects all frames' audio tokens, so the talk
forward on shards — in-process (forward_local) and with real process groups — gives the single-rank bits, as the other shard tests do
(tests/test_gpu_sp.py).  The stacked CFG pair keeps refusing the talk variant: its branches differ in their audio."""
import pytest
import torch

import synth
from gpu_util import dev, report

pytestmark = pytest.mark.gpu

# TINY_DIT_TALK widened to four heads, as test_gpu_sp.py widens TINY_DIT to WIDE_I2V
WIDE_TALK = dict(synth.TINY_DIT_TALK, dim=512, ffn_dim=768)
KPF = 32                       # audio tokens per latent frame


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------
def _frames_case(seed, rpf, heads, row0, nrows):
    D = heads * 128
    frames = (row0 + nrows - 1) // rpf + 2                       # one frame more than the range touches: a wrong frame index reads real keys
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = torch.randn((nrows, D), generator=g, device="cuda").to(torch.bfloat16)
    k = torch.randn((frames * KPF, D), generator=g, device="cuda").to(torch.bfloat16)
    vt = torch.randn((D, frames * KPF), generator=g, device="cuda").to(torch.bfloat16)
    return q, k, vt, D, frames


def _segments(row0, nrows, rpf):
    """(frame, first row, end row) of every frame segment of [row0, row0 + nrows), rows relative to row0."""
    out = []
    fr = row0 // rpf
    while fr * rpf < row0 + nrows:
        out.append((fr, max(fr * rpf, row0) - row0, min((fr + 1) * rpf, row0 + nrows) - row0))
        fr += 1
    return out


@pytest.mark.parametrize("rpf,heads,row0,nrows", [
    (24, 4, 10, 60),            # starts and ends mid-frame
    (24, 1, 5, 10),             # shorter than one frame
    (24, 40, 0, 72),
    (70, 4, 35, 105),           # odd shard of the (3, 5, 14) grid
    (70, 1, 140, 70),
    (320, 4, 100, 700),         # frames longer than a 128-row tile, not a multiple of it
    (320, 40, 130, 50),
    (1560, 40, 780, 3120),      # the 832x480 frame (30 x 52), a shard cut at half a frame
    (1560, 4, 0, 4680),
    (1560, 1, 1000, 300),
])
def test_frame_attention_is_the_per_frame_launches(rpf, heads, row0, nrows):
    from svi_hip import _lib as L
    from svi_hip import ops
    q, k, vt, D, frames = _frames_case(rpf * 7 + heads + row0, rpf, heads, row0, nrows)
    got = ops.frame_attention(q, k, vt, heads, rpf, KPF, row0=row0)
    want = torch.full_like(got, float("nan"))
    for fr, a, b in _segments(row0, nrows, rpf):
        L.check(L.lib().svi_attention_vt_fwd(q.data_ptr() + a * D * 2, D, k.data_ptr() + fr * KPF * D * 2, D, vt.data_ptr() + fr * KPF * 2,
                                             vt.shape[1], want.data_ptr() + a * D * 2, D, b - a, KPF, heads, 0, L.current_stream()),
                "svi_attention_vt_fwd")
    torch.cuda.synchronize()
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, want)
    # fp64 attention over each row's own frame, scale head_dim^-0.5
    ref = torch.empty((nrows, D), dtype=torch.float64, device="cuda")
    for fr, a, b in _segments(row0, nrows, rpf):
        qq = q[a:b].double().view(b - a, heads, 128).transpose(0, 1)
        kk = k[fr * KPF:(fr + 1) * KPF].double().view(KPF, heads, 128).transpose(0, 1)
        vv = vt[:, fr * KPF:(fr + 1) * KPF].double().view(heads, 128, KPF).transpose(1, 2)
        p = torch.softmax(qq @ kk.transpose(1, 2) / 128 ** 0.5, dim=-1)
        ref[a:b] = (p @ vv).transpose(0, 1).reshape(b - a, D)
    rel = float((got.double() - ref).norm() / ref.norm())
    report("frame_attention", rpf=rpf, heads=heads, row0=row0, nrows=nrows, rel_l2_fp64=rel)
    assert rel <= 6e-3, rel


def test_frame_attention_refuses_bad_operands():
    from svi_hip import _lib as L
    q, k, vt, D, frames = _frames_case(1, 24, 1, 0, 48)
    lib = L.lib()
    out = torch.empty_like(q)
    args = lambda row0, nrows, rpf, kpf, ldvt: (q.data_ptr(), D, k.data_ptr(), D, vt.data_ptr(), ldvt, out.data_ptr(), D, row0, nrows, rpf, kpf, 1,  # noqa: E731
                                                L.current_stream())
    assert lib.svi_attention_frames_fwd(*args(0, 48, 24, KPF, frames * KPF)) == 0
    assert lib.svi_attention_frames_fwd(*args(0, 48, 24, 12, frames * KPF)) != 0          # keys per frame not a multiple of 8
    assert "multiple of 8" in L.last_error()
    assert lib.svi_attention_frames_fwd(*args(0, 48, 24, KPF, KPF)) != 0                  # V^T does not hold the touched frames' keys
    assert lib.svi_attention_frames_fwd(*args(-1, 48, 24, KPF, frames * KPF)) != 0
    assert lib.svi_attention_frames_fwd(*args(0, 48, 0, KPF, frames * KPF)) != 0
    torch.cuda.synchronize()


# ---- 2. the talk forward on shards, in one process ---------------------------------------------------------------------------------
def handles(hip, c, seed, n):
    sd = {k: torch.from_numpy(v).to("cuda", torch.bfloat16).contiguous() for k, v in synth.dit_state_dict(seed, **c).items()}
    out = []
    for _ in range(n):
        m = hip.WanDiT(eps=1e-6, num_heads=synth.num_heads_of(c), **c)
        m.bind(sd)
        out.append(m)
    return out


def talk_inputs(seed, grid, with_addc=False):
    f, h, w = grid
    x = dev(synth.randn(seed + 1, 1, 16, f, 2 * h, 2 * w))
    ctx = dev(synth.text_context(seed + 2, 16, 64, 9))
    kw = dict(clip_feature=dev(synth.randn(seed + 3, 1, 257, 1280)), y=dev(synth.randn(seed + 4, 1, 20, f, 2 * h, 2 * w)))
    if with_addc:
        kw["add_condition"] = dev(0.1 * synth.randn(seed + 6, 1, f * h * w, WIDE_TALK["dim"]))
    aud = tuple(dev(a) for a in synth.audio_windows(seed + 5, f))
    return x, ctx, kw, aud


# grids: (3, 4, 6) = 24-row frames (cuts mid-frame at P = 2 and 4), (3, 5, 14) = 70-row frames (P = 2: odd 105-row shards), (3, 10, 16) = 160-row
# frames, longer than a 128-row tile (P = 2 and 4 cut them)
@pytest.mark.parametrize("P,G,grid,addc", [(P, G, g, a) for g in [(3, 4, 6), (3, 5, 14), (3, 10, 16)]
                                           for P, G in [(1, 1), (1, 2), (2, 1), (2, 2), (4, 1)] if (g[0] * g[1] * g[2]) % P == 0
                                           for a in (False, True)])
def test_talk_forward_on_shards_is_bit_identical(P, G, grid, addc):
    import svi_hip
    from svi_hip import sequence_parallel as sp
    ms = handles(svi_hip, WIDE_TALK, 930, P + 1)
    x, ctx, kw, aud = talk_inputs(931, grid, addc)
    t = torch.tensor([637.5])
    want = svi_hip.model_fn_wan_talk_video(ms[-1], x, t, ctx, audio_embed_tuple=aud, **kw).clone()
    got = sp.forward_local(ms[:P], x, t, ctx, groups=G, audio_embed_tuple=aud, **kw)
    assert got.shape == want.shape and torch.isfinite(got.float()).all()
    assert torch.equal(got, want)
    assert all(m._audio is None for m in ms)                        # armed for the call only
    plain = sp.forward_local(ms[:P], x, t, ctx, groups=G, **kw)     # the audio branch is really in the shard result
    assert not torch.equal(plain, want)
    again = sp.forward_local(ms[:P], x, t, ctx, groups=G, audio_embed_tuple=aud, **kw)      # reused exchange and audio buffers
    assert torch.equal(again, want)


@pytest.mark.parametrize("grid,exact", [((4, 12, 16), True), ((3, 4, 6), False)])
def test_talk_forward_in_gather_mode(grid, exact):
    """4 heads over 3 ranks: the K / V all-gather mode.  Its self-attention regroups rows into wavefronts from the shard's first row (test_gpu_sp.py:
    bit for bit when the shard length is a multiple of 256, else within 3e-3); the audio attention on the shards adds no difference of its own.
    (4, 12, 16): 192-row frames, 256-row shards cut frames 1 and 2."""
    import svi_hip
    from svi_hip import sequence_parallel as sp
    ms = handles(svi_hip, WIDE_TALK, 930, 4)
    x, ctx, kw, aud = talk_inputs(941, grid, True)
    t = torch.tensor([412.0])
    want = svi_hip.model_fn_wan_talk_video(ms[-1], x, t, ctx, audio_embed_tuple=aud, **kw).clone()
    got = sp.forward_local(ms[:3], x, t, ctx, mode="gather", audio_embed_tuple=aud, **kw)
    assert got.shape == want.shape and torch.isfinite(got.float()).all()
    rel = float((got.float() - want.float()).norm() / want.float().norm())
    assert rel < 3e-3, rel
    if exact:
        assert (grid[0] * grid[1] * grid[2] // 3) % 256 == 0 and torch.equal(got, want)


# ---- 4. what stays refused ----------------------------------------------------------------------------------------------------------
def test_talk_refusals_on_shards():
    import svi_hip
    from svi_hip import _lib as L
    from svi_hip import sequence_parallel as sp
    grid = (3, 4, 6)
    ms = handles(svi_hip, WIDE_TALK, 930, 3)
    x, ctx, kw, aud = talk_inputs(951, grid)
    neg = dev(synth.text_context(957, 16, 64, 4))
    t = torch.tensor([637.5])
    for m in ms:
        m.context_cache(True)
        m.set_audio(aud)
    try:
        with pytest.raises(RuntimeError, match="audio"):               # the stacked CFG pair on a shard
            sp.forward_local_pair(ms[:2], x, t, ctx, neg, **kw)
        with pytest.raises(RuntimeError, match="audio"):               # and on one rank
            ms[-1].forward_cfg_pair(x, t, ctx, neg, **kw)
    finally:
        for m in ms:
            m.set_audio(None)
            m.context_cache(False)
    # audio windows for another frame count: refused on a shard as on one rank, by the Python layer ...
    short = tuple(dev(a) for a in synth.audio_windows(958, grid[0] - 1))
    with pytest.raises(ValueError, match="latent frames"):
        svi_hip.model_fn_wan_talk_video(ms[-1], x, t, ctx, audio_embed_tuple=short, **kw)
    with pytest.raises(ValueError, match="latent frames"):
        sp.forward_local(ms[:2], x, t, ctx, audio_embed_tuple=short, **kw)
    assert ms[0]._audio is None and ms[1]._audio is None
    # ... and by the library itself: the windows are checked against the WHOLE sequence's frames, whichever frames the shard's rows cover
    m = ms[0]
    m.set_audio(short)
    try:
        B, _, T, H, W = x.shape
        xb, ts, ctxb = x.contiguous(), torch.tensor([637.5], device="cuda"), ctx.contiguous()
        st = L.current_stream()
        L_ = grid[0] * grid[1] * grid[2]
        for row0, nrows in ((0, L_ // 2), (L_ // 2, L_ // 2), (0, grid[1] * grid[2])):
            rc = L.lib().svi_dit_sp_begin(m._h, xb.data_ptr(), ts.data_ptr(), ctxb.data_ptr(), kw["clip_feature"].data_ptr(), kw["y"].data_ptr(), None,
                                          T, H, W, ctxb.shape[1], row0, nrows, st)
            assert rc != 0 and "audio windows cover 2 latent frames, the latents have 3" in L.last_error(), (rc, L.last_error())
    finally:
        m.set_audio(None)
    torch.cuda.synchronize()


# ---- 3. across processes ------------------------------------------------------------------------------------------------------------
def _dist_worker(rank, world, port, queue):
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)       # all ranks share the one GPU; gloo moves the exchanges through the host
    try:
        import svi_hip
        torch.cuda.set_device(0)
        m = handles(svi_hip, WIDE_TALK, 930, 1)[0]
        grid = (3, 4, 6)                                                # 72 tokens: 36-row shards at world 2, 18-row ones at 4 (cut mid-frame)
        x, ctx, kw, aud = talk_inputs(961, grid, True)
        t = torch.tensor([637.5])
        want = svi_hip.model_fn_wan_talk_video(m, x, t, ctx, audio_embed_tuple=aud, **kw).clone()
        got = svi_hip.model_fn_wan_talk_video(m, x, t, ctx, audio_embed_tuple=aud, use_unified_sequence_parallel=True, **kw)
        rel = lambda a, b: float((a.float() - b.float()).norm() / b.float().norm())      # noqa: E731
        r_fwd = rel(got, want) if m._audio is None else 1.0
        # TeaCache + shards: the same skip pattern, this rank's [Ls, dim] residual rows, the single-rank bits.  A huge threshold makes every
        # middle step a skip; step 0 and the last one compute
        outs = {}
        for usp in (False, True):
            tc = svi_hip.TeaCache(5, 1e9, "Wan2.1-I2V-14B-480P")
            xs, pattern = x.clone(), []
            for i in range(5):
                o = svi_hip.model_fn_wan_talk_video(m, xs, torch.tensor([500.0 + 0.01 * i]).cuda(), ctx, tea_cache=tc, audio_embed_tuple=aud,
                                                    use_unified_sequence_parallel=usp, **kw)
                pattern.append(tuple(tc.previous_residual.shape))
                xs = (xs.float() + 0.05 * o.float()).to(torch.bfloat16)
            outs[usp] = (xs, tuple(pattern))
        Ls = grid[0] * grid[1] * grid[2] // world
        r_tea = rel(outs[True][0], outs[False][0]) if outs[True][1] == ((Ls, WIDE_TALK["dim"]),) * 5 else 1.0
        # the three-forward talk sampler on shards
        f, h, w = grid
        lat = svi_hip.generate_noise((1, 16, f, 2 * h, 2 * w), seed=31, device="cpu", dtype=torch.float32)
        null = tuple(dev(a) for a in synth.audio_windows(967, f))
        neg = dev(synth.text_context(968, 16, 64, 4))
        sk = dict(num_inference_steps=3, text_scale=5.0, audio_scale=4.0, **kw)
        ref = svi_hip.DenoiseLoop(m).sample_multitalk(dev(lat), ctx, neg, aud, null, **sk)
        out = svi_hip.DenoiseLoop(m, sequence_parallel=True).sample_multitalk(dev(lat), ctx, neg, aud, null, **sk)
        r_loop = rel(out, ref) if bool(torch.isfinite(out.float()).all()) else 1.0
        queue.put((rank, r_fwd, r_tea, r_loop))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_talk_across_processes(world):
    """model_fn_wan_talk_video(use_unified_sequence_parallel=True), a TeaCache talk sequence on shards (same skip pattern, [Ls, dim] residuals) and
    DenoiseLoop(sequence_parallel=True).sample_multitalk with a real process group (one process per rank) against the single-rank runs.
    The ranks share the test box's one GPU, and two processes on one GPU make even REPEATED single-rank forwards differ in a last bit now and
    then (the parent tree's plain I2V forward included; one process alone is deterministic), so across processes the bounds are tolerances: 3e-3
    for a forward and the TeaCache sequence (measured: 0 on every rank so far), and test_gpu_talk.py's sampler bound 5e-2 for three sampler steps,
    where guidance scales of 5 and 4 carry a last-bit difference on (measured: up to 1.03e-2).  The bit-for-bit statement is the in-process tests'."""
    from spawn_util import run_ranks
    res = run_ranks(_dist_worker, world, timeout=300)
    report(f"talk_across_processes_{world}", ranks=[list(r) for r in sorted(res)])
    assert sorted(r[0] for r in res) == list(range(world)), res
    assert all(r[1] < 3e-3 and r[2] < 3e-3 and r[3] < 5e-2 for r in res), res
