"""The rolling-window denoising loop on the HIP backend, and `install(pipe)` — the drop-in swap.

    DenoiseLoop.sample(...)     <- SVIVideoPipeline._sample_with_regular_video   pipelines/svi_video.py:392-421
                                   (== the loop in WanVideoPipeline.__call__, pipelines/wan_video.py:266-278)
    generate_noise(...)         <- BasePipeline.generate_noise                  pipelines/base.py:140-143
    install(pipe)               <- the reference's own swap idioms: module-attribute / bound-method rebinding
                                   (pipelines/svi_video.py:265-273 does the same for USP)
"""
from __future__ import annotations

import contextlib
import sys
import types
import weakref
from typing import Callable, Dict, Optional

import torch

from . import _lib as L
from . import ops
from .dit import WanDiT, _version, model_fn_wan_video
from .scheduler import FlowMatchScheduler


def generate_noise(shape, seed=None, device="cpu", dtype=torch.float16):
    """Seeded noise comes from torch's CPU generator in the reference; keeping that is what makes seeds portable."""
    generator = None if seed is None else torch.Generator(device).manual_seed(seed)
    return torch.randn(shape, generator=generator, device=device, dtype=dtype)


def _release_stream_buffers(stream) -> bool:
    """True when the library's buffers of `stream` were released (False: a capture is running on this thread — the release drains the device — or the
    device / library is gone)."""
    try:
        if torch.cuda.is_current_stream_capturing():      # the release drains the device: illegal inside another loop's capture — leave the buffers
            return False
        L.release_stream_buffers(stream)
        return True
    except Exception:      # a finalizer must not raise (device gone, library unloaded)
        return False


# TeaCache steps under `graph=None` (the default) take the graphed path, as every other step of the single-rank loop does; `graph=False` keeps the eager
# path through model_fn_wan_video.  Decided by the alternating A/B of tools/teacache_graph_ab.py: the clip median is lower at the C1 and at the C2 size
# (profiles/teacache_graph_ab.txt).
TEA_GRAPH_BY_DEFAULT = True

# The talk step with TeaCache has one captured graph per mode triple (cond, uncond, drop-text).  A positive and a negative cache can produce all eight
# triples of {store, skip}; a clip lives on few of them: the step on which everything computes — (1, 1, 1), or (1, 1, 2) when the negative cache's second
# check of the step, on an unchanged t_mod, already skips —, the all-skip step (2, 2, 2), and a transitional triple or two where the negative cache, which is
# consulted twice per step and so fills its budget sooner, computes a step before the positive one.  Four graphs hold these; a fifth triple evicts the
# least recently used one, which is captured again if it returns (tests/test_gpu_talk3_tea.py cycles through more).
TALK_TEA_GRAPHS = 4


class _Clip:
    """What DenoiseLoop.clip() yields: the tensors one clip's steps run on."""

    def __init__(self, latents, ctx_pos, ctx_neg, cond, resident):
        self.latents, self.ctx_pos, self.ctx_neg, self.cond, self.resident = latents, ctx_pos, ctx_neg, cond, resident

    def result(self) -> torch.Tensor:
        """The denoised latents: a resident loop's slot is the next clip's too, so a copy."""
        return self.latents.clone() if self.resident else self.latents


class DenoiseLoop:
    """50 x { cond forward, uncond forward, CFG combine, Euler step } with latents resident in HBM."""

    def __init__(self, dit: WanDiT, scheduler: Optional[FlowMatchScheduler] = None, cfg_pair=None, sp_group=None, sequence_parallel: bool = False,
                 graph: Optional[bool] = None, resident: bool = False):
        """`cfg_pair`: an svi_hip.parallel.CfgPair — this rank then runs only its half of every CFG pair of forwards.
        `sequence_parallel` (+ `sp_group`, default: the world): every forward is spread Ulysses-style over the ranks of the group
        (svi_hip/sequence_parallel.py); all of them hold the full latents and apply the same CFG/Euler update.
        `graph`: the two forwards of a step are captured ONCE into a hipGraph (through torch.cuda.CUDAGraph) and replayed for every
        later step of the clip — the ~1500 launches of a step become one; the timestep is read from a device scalar that is
        refreshed before each replay.  Decisive where a step is launch-bound (BASELINE configs[0]: 1280 tokens), still 1.1 % at the
        C2 size (profiles/r3m_prof_events_ab.txt); results are bit-identical (the same kernels on the same operands).  Single-rank
        path only.  Default (None): ON for the single-rank loop, off with a CFG pair / sequence parallelism (their
        exchanges are host-driven).  The first step of a clip runs eagerly on the capture stream — it IS that step — and is recorded
        right behind itself; steps 2.. replay.
        With TeaCache (step()'s tea_cache_posi / _nega) a graphed loop keeps its fast path: the skip decisions are taken on the host from t_mod, as
        ever, and the step's device work — one forward_cfg_pair(tea_mode) call, or two forward(tea_mode) calls where the branches cannot share — is
        captured once per mode (computed / skipped) and replayed; a resident loop stays resident.  Bit-identical to the eager TeaCache path
        (tests/test_gpu_teacache_graph.py).  `graph=True` selects it, `graph=False` keeps the eager path through model_fn_wan_video; under
        `graph=None` TEA_GRAPH_BY_DEFAULT decides (profiles/teacache_graph_ab.txt).
        `resident` (the rolling-window drivers turn it on: StreamLoop, install()'s sampler, bench.py --window): the loop OWNS the device tensors
        a clip's steps read — latents, the two prompt embeddings, clip_feature, y, add_condition — and every clip's inputs are copied into them
        (adopt()).  A clip boundary then moves no address: the prompt's cache entries are recomputed in place (WanDiT.refill_context) and the step
        graph captured for the first clip of a stream is replayed by every later clip of the same shapes — no eager step, no re-capture, no
        re-instantiation per clip.  The context cache stays on while the loop lives (close() turns it off).  Same kernels on the same values:
        bit-identical to the non-resident loop (tests/test_gpu_stream.py).
        The talk variant (sample_multitalk) is on the same path: with `graph` on, a step is ONE forward_talk3 call — the three guidance forwards, their
        shared prefix computed once, the audio K / V^T of every block projected once per clip into the DiT's audio slots — captured on the clip's first
        step and replayed; a resident loop re-stages the slots in place at a clip boundary and keeps replaying.  `graph=False` keeps the three eager
        model_fn_wan_talk_video calls per step.  Bit-identical either way (tests/test_gpu_talk3.py)."""
        self.dit = dit
        self.cfg_pair = cfg_pair
        self.sequence_parallel, self.sp_group = sequence_parallel, sp_group
        self.scheduler = scheduler or FlowMatchScheduler(shift=5, sigma_min=0.0, extra_one_step=True)
        self._cond = self._uncond = self._drop = None      # the step's noise predictions (the talk step has a third: drop-text)
        if graph and (cfg_pair is not None or sequence_parallel):
            raise ValueError("graph capture covers the single-rank step only")
        self.graph = (cfg_pair is None and not sequence_parallel) if graph is None else bool(graph)
        self.resident = bool(resident) and self.graph
        self.tea_graph = self.graph and (TEA_GRAPH_BY_DEFAULT if graph is None else True)      # TeaCache steps on the graphed path (else: model_fn_wan_video)
        self._slots: Dict[str, torch.Tensor] = {}      # resident: name -> the loop's own tensor of that input
        self._slot_src: Dict[str, tuple] = {}          # name -> (the tensor last copied in — kept alive so that its address cannot return as another's —, its version)
        self.last_sp_form = None      # sequence-parallel steps: "stacked pair" (forward_distributed_pair) or "two forwards"
        self.captures = 0             # how many times a step was captured (a resident stream of equal-shaped clips: once)
        self._graph = None            # dict(key, graph, ts, pins, generation) of the captured step, see _forwards_graphed
        self._tea_graphs: Dict[tuple, dict] = {}      # TeaCache: (mode of the conditional branch, of the unconditional) -> the same dict; at most two alive
        self._tea_res: Dict[str, torch.Tensor] = {}   # the loop's residual tensor per branch (a resident loop keeps them in _slots: their addresses survive a clip boundary)
        self.tea_counts = {"computed": 0, "skipped": 0}      # TeaCache steps since the last sample() began, by the conditional branch's decision
        self.talk_tea_counts: Dict[tuple, int] = {}          # the talk loop's TeaCache steps since the last clip began, by mode triple (cond, uncond, drop-text)
        self._capture_stream = None   # ONE side stream per loop, reused by every re-capture: the library keeps per-stream scratch (flag words,
                                      # split-K partials) for good, so a fresh pool stream per capture would multiply it

    def _forwards(self, latents, timestep, ctx_pos, ctx_neg, cfg_scale, split, cond, ucond, tea=None) -> None:
        """The DiT forward(s) of one step into self._cond / self._uncond.  `tea`: (tea_mode, residual) of the conditional branch, then of the unconditional
        one (_tea_decide) — one pair call when the branches can share and decided alike, else one forward per branch with its own mode."""
        mc, rc, mu, ru = tea or (0, None, 0, None)
        tc = dict(tea_mode=mc, residual=rc) if mc else {}
        if cfg_scale != 1.0:
            if ctx_neg.shape == ctx_pos.shape and not split and mc == mu:      # one call: the prompt-independent head of the forward is shared, results unchanged
                tp = dict(tea_mode=mc, residual_cond=rc, residual_uncond=ru) if mc else {}
                self.dit.forward_cfg_pair(latents, timestep, ctx_pos, ctx_neg, out_cond=self._cond, out_uncond=self._uncond, **tp, **cond)
            else:
                tu = dict(tea_mode=mu, residual=ru) if mu else {}
                self.dit.forward(latents, timestep, ctx_pos, out=self._cond, **tc, **cond)
                self.dit.forward(latents, timestep, ctx_neg, out=self._uncond, **tu, **ucond)
        else:
            self.dit.forward(latents, timestep, ctx_pos, out=self._cond, **tc, **cond)

    def _tea_residual(self, name: str, shape, device) -> torch.Tensor:
        """The loop's own residual tensor of one branch; in resident mode a slot (kept from clip to clip, so a captured step's addresses hold)."""
        store, key = (self._slots, "tea_residual_" + name) if self.resident else (self._tea_res, name)
        res = store.get(key)
        if res is None or tuple(res.shape) != tuple(shape) or res.device != device:
            res = store[key] = torch.empty(shape, dtype=torch.bfloat16, device=device)
        return res

    def _tea_decide(self, latents, timestep, caches):
        """The TeaCache decisions of one step, on the host, before anything of the step is enqueued: each object's own check(dit, token, t_mod)
        (svi_hip.TeaCache or the reference's class, svi_video.py:43-62) on this step's t_mod.  Returns (mode, residual) per branch, flattened:
        2 + the object's previous_residual for a skip, 1 + the loop's residual tensor of that branch for a computed step, (0, None) without an object."""
        t_mod = self.dit.time_mod(timestep)
        B, _, T, H, W = latents.shape
        shape = (B, self.dit.tokens(T, H, W), self.dit.dim)
        out = []
        for name, cache in zip(("cond", "uncond"), caches):
            if cache is None:
                out += [0, None]
            elif cache.check(self.dit, t_mod[:, :1, :1], t_mod):      # the token: check() keeps `x` only for a residual that is formed on the device here
                res = cache.previous_residual
                if res is None:
                    raise RuntimeError("TeaCache asked to skip before any residual was stored")
                out += [2, res]
            else:
                out += [1, self._tea_residual(name, shape, latents.device)]
        self.tea_counts["skipped" if out[0] == 2 else "computed"] += 1
        return tuple(out)

    def adopt(self, latents: torch.Tensor, ctx_pos: torch.Tensor, ctx_neg: Optional[torch.Tensor], cond: dict):
        """Resident mode: copy one clip's inputs into the loop's own tensors and return those (latents, ctx_pos, ctx_neg, cond).  A tensor whose
        shape changed gets a new slot (the next step re-captures); a prompt-side tensor (prompt embeddings, clip_feature) that is the very tensor
        copied last time, unmodified, is not copied again; when one did change, the context-cache entries keyed by the slots are recomputed in place."""
        dev = latents.device

        def put(name, src, prompt_side=False):
            if src is None:
                self._slots.pop(name, None)
                self._slot_src.pop(name, None)
                return None, False
            slot = self._slots.get(name)
            last = self._slot_src.get(name)
            fresh = slot is None or slot.shape != src.shape or slot.device != dev
            if not fresh and prompt_side and last is not None and last[0] is src and last[1] == _version(src):
                return slot, False
            if fresh:
                slot = self._slots[name] = torch.empty(src.shape, dtype=torch.bfloat16, device=dev)
            slot.copy_(src)
            self._slot_src[name] = (src, _version(src)) if prompt_side else None
            return slot, not fresh
        lat, _ = put("latents", latents)
        cp, r0 = put("ctx_pos", ctx_pos, True)
        cn, r1 = put("ctx_neg", ctx_neg, True)
        out = {}
        r2 = False
        for k, v in cond.items():
            if isinstance(v, torch.Tensor):
                out[k], r = put(k, v, prompt_side=(k == "clip_feature"))
                r2 = r2 or (r and k == "clip_feature")
            else:
                out[k] = v
        cf = out.get("clip_feature") if self.dit.has_image_input else None
        if self.dit._ctx_cache_on:
            # in-place writes into tensors the cache knows: recompute their entries where they stand (a slot that was just created is simply a miss)
            if (r0 or r2) and cp is not None:
                self.dit.refill_context(cp, cf)
            if (r1 or r2) and cn is not None:
                self.dit.refill_context(cn, cf)
        return lat, cp, cn, out

    def _owned(self, t) -> bool:
        return self.resident and t is not None and any(t is s for s in self._slots.values())

    def stays_resident(self, tea: bool) -> bool:
        """Whether a clip runs on the loop's own tensors: a resident loop, unless the clip's TeaCache steps take step()'s eager path."""
        return self.resident and (not tea or self.tea_graph)

    @contextlib.contextmanager
    def clip(self, latents: torch.Tensor, ctx_pos: torch.Tensor, ctx_neg: Optional[torch.Tensor], cond: dict, resident: bool,
             convert: Optional[Callable] = None, every_cond: bool = False, keep_cache: bool = False, audio_slots: bool = False):
        """A clip's begin and end around its steps.  Yields a _Clip: the tensors the steps run on, and result() for what the clip returns.
        `resident`: the context cache goes on if it is off and the inputs are copied into the loop's own tensors (adopt); the end leaves everything for
        the next clip.  Otherwise the latents are cloned as contiguous bf16 (the caller's tensor stays untouched), the prompt embeddings and
        clip_feature — with `every_cond` every tensor of `cond`: a captured step reads those very tensors — go through `convert` (default: contiguous
        bf16 on the latents' device; install()'s samplers pass _stable_bf16), and the end drops the captured step, which read this clip's tensors and
        cache entries.  `keep_cache` (install()'s samplers): the context cache is left as it is when on, and left on at the end; else it is switched
        on for the clip and off behind it.  `audio_slots`: the talk clip's two staged slots go with the clip too."""
        dit = self.dit
        if resident:
            if not dit._ctx_cache_on:
                dit.context_cache(True)
            run = _Clip(*self.adopt(latents, ctx_pos, ctx_neg, cond), resident=True)
        else:
            lat = latents.to(torch.bfloat16).contiguous().clone()
            conv = convert or (lambda t: None if t is None else t.to(device=lat.device, dtype=torch.bfloat16).contiguous())
            ctx_pos, ctx_neg = conv(ctx_pos), conv(ctx_neg)
            cond = {k: conv(v) if isinstance(v, torch.Tensor) and (every_cond or k == "clip_feature") else v for k, v in cond.items()}
            run = _Clip(lat, ctx_pos, ctx_neg, cond, resident=False)
            if not (keep_cache and dit._ctx_cache_on):
                dit.context_cache(True)
        try:
            yield run
        finally:
            if not resident:
                self.drop_graph()
                if audio_slots:
                    dit.stage_audio(0, None)
                    dit.stage_audio(1, None)
                if not keep_cache:
                    dit.context_cache(False)

    def close(self) -> None:
        """End of a resident stream: the captured step, the slots and the context cache go."""
        self._graph = None
        self._tea_graphs.clear()
        self._slots, self._slot_src = {}, {}
        for slot in list(self.dit._audio_slots):         # a talk stream's audio slots (about 0.55 GB each at the 14B width)
            self.dit.stage_audio(slot, None)
        if self.resident and self.dit._ctx_cache_on:
            self.dit.context_cache(False)
        self._retire_capture_stream()                    # the stream's end also ends its capture stream and the library's buffers keyed to it

    def held_graphs(self) -> list:
        """The captured graphs the loop holds now (the plain step's, then the TeaCache ones): a stream that replays holds the same objects clip after clip."""
        return ([self._graph["graph"]] if self._graph is not None else []) + [h["graph"] for h in self._tea_graphs.values()]

    def drop_graph(self) -> None:
        """Forget the captured step (a later graphed step captures again)."""
        self._graph = None
        self._tea_graphs.clear()

    def _retire_capture_stream(self) -> bool:
        """Release the library's per-stream buffers of this loop's capture stream and forget the stream.  When the release cannot happen now (another loop's
        capture is running on this thread) the stream AND its finalizer are kept: a later release() / close() / garbage collection still frees the ~100 MB the
        library holds for it at the C2 size (the finalizer used to be spent by the skipped attempt)."""
        fin = getattr(self, "_stream_finalizer", None)
        st = self._capture_stream
        if st is None:
            return True
        if not _release_stream_buffers(st):
            return False
        if fin is not None:
            fin.detach()                                 # the buffers are gone: nothing left for the finalizer to do
        self._stream_finalizer = None
        self._capture_stream = None
        return True

    def release(self) -> None:
        """Retire this loop's capture stream: the captured step and the library's per-stream buffers keyed to that stream are freed
        (also done when the loop is garbage-collected)."""
        self._graph = None
        self._tea_graphs.clear()
        self._retire_capture_stream()

    def _graph_key(self, latents, ctx_pos, ctx_neg, cfg_scale, split, cond, tea=None):
        """(slot, key, tensors) of a step's captured graph: which graph of the loop serves the step (None: the plain step; with TeaCache the pair of
        the branches' modes), what must still hold for a replay, and the tensors the graph pins.  See _forwards_graphed."""
        def ident(t):      # the loop's own tensors (resident mode) are rewritten by adopt() between clips: their version is not part of the key
            return None if t is None else (t.data_ptr(), tuple(t.shape), t.dtype, -1 if self._owned(t) else _version(t))
        tensors = [latents, ctx_pos, ctx_neg, self._cond, self._uncond] + [v for _, v in sorted(cond.items()) if isinstance(v, torch.Tensor)]
        slot = None if tea is None else (tea[0], tea[2])
        residuals = [] if tea is None else [tea[1], tea[3]]
        key = (tuple(ident(t) for t in tensors), tuple(sorted((k, None if isinstance(v, torch.Tensor) else repr(v)) for k, v in cond.items() if v is not None)),
               float(cfg_scale), bool(split), self.dit.epoch(), L.switch_epoch())
        if tea is not None:
            key += (slot, tuple(None if r is None else (r.data_ptr(), tuple(r.shape), r.dtype) for r in residuals))
        return slot, key, tensors + [r for r in residuals if r is not None]

    def _forwards_graphed(self, latents, timestep, ctx_pos, ctx_neg, cfg_scale, split, cond, ucond, tea=None) -> None:
        """Replay (capture on first use) the hipGraph of this step's forwards.

        A captured graph has baked in the ADDRESSES of everything it reads and writes (latents, prompt embeddings, conditioning
        tensors, output buffers, the DiT workspace, the context-cache entries) and a context-cache HIT (the projected prompt and every
        block's cross-attention K / V are read, never recomputed).  So a replay is only legal while all of that still holds:
          * the graph keeps STRONG references to every tensor it reads (their storage cannot be recycled for another prompt), and its
            key records each one's address, shape and version counter (an in-place write makes a new key);
          * the key carries the DiT's host-side epoch (context_cache() on / off, re-bind) and the C side's generation counter
            (svi_dit_generation: workspace growth, a context entry filled or evicted) as read right after the capture;
          * the key carries the count of in-process switch reloads (_lib.set_switch): a graph recorded under other library switches is not replayed;
          * sample() drops the graph when the clip is done.
        Anything else re-captures.
        TeaCache (`tea`, see _forwards): a computed step and a skipped step are different device work, so each mode — the pair (mode of the conditional
        branch, mode of the unconditional one) — has a captured graph of its own, under the same rules; the key also carries the residual tensors'
        identities (their contents are the graphs' business: the store graph writes them, the skip graph reads them).  Two are kept at the most, and
        capturing one mode leaves the other's graph alone."""
        self.dit._refresh_if_weights_changed()          # a LoRA merge since the last step re-binds (and moves the epoch) BEFORE the key is formed
        slot, key, tensors = self._graph_key(latents, ctx_pos, ctx_neg, cfg_scale, split, cond, tea)
        self._replay_or_capture(slot, key, tensors, latents.device, timestep,
                                lambda ts: self._forwards(latents, ts, ctx_pos, ctx_neg, cfg_scale, split, cond, ucond, tea))

    def _held_graph(self, slot, lru: bool = False):
        """The graph held under `slot` (None: the plain step's), or None; with `lru` the look-up counts as a use."""
        if slot is None:
            return self._graph
        held = self._tea_graphs.get(slot)
        if lru and held is not None:
            self._tea_graphs[slot] = self._tea_graphs.pop(slot)      # most recently used: last
        return held

    def _keep_tea_graph(self, slot, held, bound: int) -> None:
        """Hold a TeaCache graph under `slot`, at most `bound` of them: the first in the dict's order goes (the oldest capture; the least recently used
        one where the look-ups count as uses)."""
        self._graph = None
        self._tea_graphs.pop(slot, None)
        while len(self._tea_graphs) >= bound:    # caches that disagree can ask for a third mode: the oldest goes
            self._tea_graphs.pop(next(iter(self._tea_graphs)))
        self._tea_graphs[slot] = held

    def _replay_or_capture(self, slot, key, tensors, device, timestep, run, bound: int = 2, lru: bool = False) -> None:
        """Replay the graph held under `slot` while `key` and the DiT's generation still hold; else run `run(timestep tensor)` eagerly on the loop's
        capture stream — it IS this step — and record it right behind itself.  See _forwards_graphed for the rules.  At most `bound` TeaCache graphs
        stay alive; with `lru` a replay counts as a use, so the one evicted is the least recently used (else the oldest capture)."""
        held = self._held_graph(slot, lru)
        stale = held is None or held["key"] != key or held["generation"] != self.dit.generation()
        if stale:
            if slot is None:
                self._graph = None
            else:
                self._tea_graphs.pop(slot, None)
            if self._capture_stream is None or self._capture_stream.device != device:
                self._retire_capture_stream()
                self._capture_stream = torch.cuda.Stream(device=device)
                # a loop that is simply dropped (DenoiseLoop(m).step(...)) must not leave the library's per-stream buffers (flag words, split-K
                # partials, the fp8 attention operands: ~100 MB at the C2 size) keyed to a pool stream for the life of the process
                self._stream_finalizer = weakref.finalize(self, _release_stream_buffers, self._capture_stream)
                self._stream_finalizer.atexit = False      # at interpreter exit the HIP runtime may already be gone
            side = self._capture_stream                  # eager run AND capture on one stream: the library's per-stream buffers exist before the capture
            ts_static = timestep.clone()                 # made on the current stream BEFORE the side stream is told to wait for it: the eager step reads it
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                # this step itself, eagerly: it also sizes the workspaces, fills the context cache and creates the flag words,
                # so that the recording below allocates nothing
                run(ts_static)
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            # recorded, not executed: self._cond / self._uncond keep the eager step's results.  thread_local: other threads of the process (a
            # communicator's watchdog, a data loader) are not bound by this capture's rules
            with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                run(ts_static)
            torch.cuda.current_stream().wait_stream(side)
            held = dict(key=key, graph=g, ts=ts_static, pins=tensors, generation=self.dit.generation())
            if slot is None:
                self._graph = held
                self._tea_graphs.clear()                 # a loop is used with TeaCache or without: the other kind's graphs go
            else:
                self._keep_tea_graph(slot, held, bound)
            self.captures += 1
            return
        held["ts"].copy_(timestep)
        held["graph"].replay()

    def step(self, latents: torch.Tensor, timestep: torch.Tensor, dsigma: float, ctx_pos: torch.Tensor,
             ctx_neg: Optional[torch.Tensor], cfg_scale: float, tea_cache_posi=None, tea_cache_nega=None, cond_wo_pose: bool = False,
             **cond) -> torch.Tensor:
        """One scheduler step, in place on `latents` (bf16 [B,16,T,H,W]).  tea_cache_posi / _nega: one TeaCache per CFG branch
        (svi_video.py:500-501).  On a loop with `tea_graph` (see __init__) their decisions are taken first (_tea_decide) and the step runs on the loop's
        own path — graphed, the pair in one call, resident; previous_residual / previous_hidden_states end as model_fn_wan_video leaves them.  Otherwise
        (graph=False, a CFG pair, sequence parallelism) the two forwards go through model_fn_wan_video separately, as in the reference.
        `add_condition` (in **cond; the dance variant's pose embedding) goes to the conditional forward only, unless `cond_wo_pose`
        (SVIDanceVideoPipeline._sample_with_dance_video, svi_video_dance.py:423-430)."""
        ucond = cond                                # keyword inputs of the unconditional forward
        if cond.get("add_condition") is not None and not cond_wo_pose:
            ucond = dict(cond, add_condition=None)
        split = ucond is not cond                   # the two branches differ in more than the prompt
        if tea_cache_posi is not None and not self.tea_graph:
            from .dit import model_fn_wan_video
            usp = {}
            if self.sequence_parallel:          # as the reference: TeaCache + USP (svi_video.py:112-131), residuals per rank
                self.dit.sp_group = self.sp_group
                usp = dict(use_unified_sequence_parallel=True)
            if self.cfg_pair is not None and cfg_scale != 1.0:
                # a CFG pair: this rank runs ONE branch with that branch's TeaCache (round 6).  The skip decision is a function of the time modulation alone
                # (svi_video.py:36-62) — the same numbers on both ranks — so the two caches decide alike, step for step, and the exchange of noise_pred never
                # waits for a forward the partner skipped differently; each cache's residual covers its own branch, as in the serial loop
                tea_mine = tea_cache_posi if self.cfg_pair.role == 0 else tea_cache_nega
                if tea_mine is None:
                    raise ValueError("a CFG pair with TeaCache needs one TeaCache per branch (tea_cache_posi and tea_cache_nega)")
                fwd_tea = lambda x, t, c, **kw: model_fn_wan_video(self.dit, x, t, c, tea_cache=tea_mine, **usp, **kw)      # noqa: E731
                return self.cfg_pair.step(fwd_tea, ops.cfg_step_, latents, timestep, dsigma, ctx_pos, ctx_neg, cfg_scale,
                                          uncond_overrides=dict(add_condition=None) if split else None, **cond)
            cpred = model_fn_wan_video(self.dit, latents, timestep, ctx_pos, tea_cache=tea_cache_posi, **usp, **cond)
            if cfg_scale != 1.0:
                upred = model_fn_wan_video(self.dit, latents, timestep, ctx_neg, tea_cache=tea_cache_nega, **usp, **ucond)
                ops.cfg_step_(latents, cpred, upred, cfg_scale, dsigma)
            else:
                ops.cfg_step_(latents, cpred, None, 1.0, dsigma)
            return latents
        fwd = lambda x, t, c, **kw: self.dit.forward(x, t, c, **kw)      # noqa: E731
        if self.sequence_parallel:
            from .sequence_parallel import forward_distributed
            fwd = lambda x, t, c, **kw: forward_distributed(self.dit, x, t, c, group=self.sp_group, **kw)      # noqa: E731
        if self.cfg_pair is not None and cfg_scale != 1.0:
            return self.cfg_pair.step(fwd, ops.cfg_step_, latents, timestep, dsigma, ctx_pos, ctx_neg, cfg_scale,
                                      uncond_overrides=dict(add_condition=None) if split else None, **cond)
        if self.sequence_parallel:
            import torch.distributed as dist
            from .sequence_parallel import forward_distributed_pair
            world = dist.get_world_size(self.sp_group)
            pt, ph, pw = self.dit.patch_size
            tokens = (latents.shape[2] // pt) * (latents.shape[3] // ph) * (latents.shape[4] // pw)
            # svi_dit_sp_begin_pair's hard bound, decided here from shapes alone (the same answer on every rank, before any collective): 2 x the shard's
            # rows of the widest activation must stay under 2 GiB (32-bit buffer offsets); beyond it the two-forwards form runs, as before the stacking
            fits = 2 * -(-tokens // world) * max(self.dit.ffn_dim, 2 * self.dit.dim) * 2 < (1 << 31)
            stackable = (cfg_scale != 1.0 and not split and self.dit._ctx_cache_on and ctx_neg is not None and ctx_neg.shape == ctx_pos.shape
                         and ctx_neg is not ctx_pos and self.dit.num_heads % world == 0 and fits)
            if stackable:
                # both branches stacked on this rank's rows: half the launches of two shard forwards, each twice as long; no CFG exchange
                cpred, upred = forward_distributed_pair(self.dit, latents, timestep, ctx_pos, ctx_neg, group=self.sp_group, **cond)
                self.last_sp_form = "stacked pair"
            else:
                cpred = fwd(latents, timestep, ctx_pos, **cond)
                upred = fwd(latents, timestep, ctx_neg, **ucond) if cfg_scale != 1.0 else None
                self.last_sp_form = "two forwards"
            ops.cfg_step_(latents, cpred, upred, cfg_scale if upred is not None else 1.0, dsigma)
            return latents
        if self._cond is None or self._cond.shape != latents.shape:
            self._cond = torch.empty_like(latents)
            self._uncond = torch.empty_like(latents)
        run = self._forwards_graphed if self.graph else self._forwards
        if tea_cache_posi is not None:
            caches = (tea_cache_posi, tea_cache_nega if cfg_scale != 1.0 else None)
            tea = self._tea_decide(latents, timestep, caches)
            run(latents, timestep, ctx_pos, ctx_neg, cfg_scale, split, cond, ucond, tea)
            for cache, mode, res in zip(caches, tea[0::2], tea[1::2]):
                if mode == 1:                          # what TeaCache.store() would have computed (svi_video.py:64-66), as model_fn_wan_video leaves it
                    cache.previous_residual = res
                    cache.previous_hidden_states = None
        else:
            run(latents, timestep, ctx_pos, ctx_neg, cfg_scale, split, cond, ucond)
        if cfg_scale != 1.0:
            ops.cfg_step_(latents, self._cond, self._uncond, cfg_scale, dsigma)
        else:
            ops.cfg_step_(latents, self._cond, None, 1.0, dsigma)
        return latents

    @torch.no_grad()
    def sample_multitalk(self, latents: torch.Tensor, ctx_pos: torch.Tensor, ctx_neg: torch.Tensor, audio_embed_tuple, audio_embed_tuple_null,
                         num_inference_steps: int = 50, text_scale: float = 5.0, audio_scale: float = 4.0, sigma_shift: float = 5.0,
                         denoising_strength: float = 1.0, progress_bar_cmd: Callable = lambda x: x, add_condition=None,
                         tea_cache_l1_thresh: Optional[float] = None, tea_cache_model_id: str = "", tea_cache_posi=None, tea_cache_nega=None,
                         **cond) -> torch.Tensor:
        """SVITalkVideoPipeline._sample_with_multitalk (svi_video_talk.py:448-463): per step three forwards — conditional (prompt, audio,
        add_condition), unconditional (negative prompt, null audio, no add_condition), drop-text (negative prompt, audio, add_condition) —
        combined as uncond + text*(cond - drop_text) + audio*(drop_text - uncond); one forward when both scales are 1.
        A loop built with sequence_parallel=True (+ sp_group) runs each of the three forwards on this rank's sequence shard
        (model_fn_wan_talk_video with use_unified_sequence_parallel): every rank ends with the full noise predictions and the same latents.
        A single-rank loop with `graph` on (the default) and three forwards to run takes the one-call step instead (_sample_talk3): same bits.
        TeaCache as SVITalkVideoPipeline.__call__ sets it up (svi_video_talk.py:541-542, 448-466): tea_cache_l1_thresh (+ tea_cache_model_id) builds one
        object for the conditional forward and ONE for the unconditional and the drop-text forward — consulted twice per step, in that order —, or the
        objects are given (tea_cache_posi / tea_cache_nega: svi_hip.TeaCache or the reference's class; None leaves that side without).  The one-call
        step serves them too (one forward_talk3(tea_modes) call per step, a graph per mode triple); one object given for BOTH sides keeps the eager
        forwards (the conditional residual would be the negative one's buffer, which the one call refuses).
        audio_embed_tuple = audio_embed_tuple_null = None (the one-call step only): the caller has staged both audio slots for this clip itself
        (WanDiT.stage_audio_windows — a talk stream's clip boundary, TalkStreamLoop)."""
        from .dit import model_fn_wan_talk_video
        if tea_cache_l1_thresh is not None and tea_cache_posi is None and tea_cache_nega is None:
            from .teacache import TeaCache
            tea_cache_posi = TeaCache(num_inference_steps, tea_cache_l1_thresh, tea_cache_model_id)
            tea_cache_nega = TeaCache(num_inference_steps, tea_cache_l1_thresh, tea_cache_model_id)
        tea = None if tea_cache_posi is None and tea_cache_nega is None else (tea_cache_posi, tea_cache_nega)
        one_call = self.graph and self.cfg_pair is None and not self.sequence_parallel and (text_scale != 1.0 or audio_scale != 1.0)
        if one_call and (tea is None or tea_cache_posi is not tea_cache_nega):
            self.scheduler.set_timesteps(num_inference_steps, denoising_strength=denoising_strength, shift=sigma_shift)
            if add_condition is not None:
                cond = dict(cond, add_condition=add_condition)
            return self._sample_talk3(latents, ctx_pos, ctx_neg, audio_embed_tuple, audio_embed_tuple_null, text_scale, audio_scale,
                                      self.scheduler.timesteps, self.scheduler.step_delta, progress_bar_cmd, cond, tea=tea)
        if audio_embed_tuple is None or audio_embed_tuple_null is None:
            raise ValueError("sample_multitalk: audio slots staged by the caller serve the one-call step only (a graphed single-rank loop with a guidance "
                             "scale other than 1); this loop's eager forwards need audio_embed_tuple and audio_embed_tuple_null")
        fn = model_fn_wan_talk_video
        if self.sequence_parallel:
            self.dit.sp_group = self.sp_group
            fn = lambda *a, **kw: model_fn_wan_talk_video(*a, use_unified_sequence_parallel=True, **kw)      # noqa: E731
        self.scheduler.set_timesteps(num_inference_steps, denoising_strength=denoising_strength, shift=sigma_shift)
        ts_dev = self.scheduler.timesteps.to(device=latents.device, dtype=torch.float32)
        aud = tuple(a.to(device=latents.device, dtype=torch.bfloat16).contiguous() for a in audio_embed_tuple)
        aud0 = tuple(a.to(device=latents.device, dtype=torch.bfloat16).contiguous() for a in audio_embed_tuple_null)
        with self.clip(latents, ctx_pos, ctx_neg, cond, resident=False) as run:      # the eager forwards read the tuples: nothing here is the loop's own
            latents, ctx_pos, ctx_neg, cond = run.latents, run.ctx_pos, run.ctx_neg, run.cond
            for i, t in enumerate(progress_bar_cmd(self.scheduler.timesteps)):
                tt, ds = ts_dev[i:i + 1], self.scheduler.step_delta(t)
                c = fn(self.dit, latents, tt, ctx_pos, add_condition=add_condition, audio_embed_tuple=aud, tea_cache=tea_cache_posi, **cond)
                if text_scale != 1.0 or audio_scale != 1.0:
                    u = fn(self.dit, latents, tt, ctx_neg, audio_embed_tuple=aud0, tea_cache=tea_cache_nega, **cond)
                    d = fn(self.dit, latents, tt, ctx_neg, add_condition=add_condition, audio_embed_tuple=aud, tea_cache=tea_cache_nega, **cond)
                    ops.cfg3_step_(latents, c, u, d, text_scale, audio_scale, ds)
                else:
                    ops.cfg_step_(latents, c, None, 1.0, ds)
        return run.result()

    def _talk3_graphed(self, latents, timestep, ctx_pos, ctx_neg, cond, tea=None) -> None:
        """The three forwards of one talk step into self._cond / _uncond / _drop: the captured forward_talk3 call replayed, captured on first use
        (_replay_or_capture, under _forwards_graphed's rules; the key is _graph_key's plus the third output — the audio slots' buffers are the DiT's:
        its generation() covers them, and a slot rewritten in place for the next clip leaves it alone).
        `tea` = (mode triple, residual per branch) of _talk_tea_decide: the triple has a graph of its own (slot ("talk3", cond, uncond, drop-text)), the
        triple and the residual tensors' identities are part of its key."""
        self.dit._refresh_if_weights_changed()          # (a re-bind drops the audio slots: forward_talk3 then refuses by name — stage them again)
        _, key, tensors = self._graph_key(latents, ctx_pos, ctx_neg, 0.0, False, cond)
        d = self._drop
        key += ("talk3", (d.data_ptr(), tuple(d.shape), d.dtype, _version(d)))
        if tea is None:
            self._replay_or_capture(None, key, tensors + [d], latents.device, timestep,
                                    lambda ts: self.dit.forward_talk3(latents, ts, ctx_pos, ctx_neg, out_cond=self._cond, out_uncond=self._uncond,
                                                                      out_drop_text=self._drop, **cond))
            return
        modes, residuals = tea
        key += (modes, tuple(None if r is None else (r.data_ptr(), tuple(r.shape), r.dtype) for r in residuals))
        self._replay_or_capture(("talk3",) + modes, key, tensors + [d] + [r for r in residuals if r is not None], latents.device, timestep,
                                lambda ts: self.dit.forward_talk3(latents, ts, ctx_pos, ctx_neg, out_cond=self._cond, out_uncond=self._uncond,
                                                                  out_drop_text=self._drop, tea_modes=modes, residual_cond=residuals[0],
                                                                  residual_uncond=residuals[1], residual_drop_text=residuals[2], **cond),
                                bound=TALK_TEA_GRAPHS, lru=True)

    def _talk_tea_decide(self, latents, timestep, tea_posi, tea_nega):
        """The TeaCache decisions of one talk step, on the host, before anything of the step is enqueued, in the reference's order (svi_video_talk.py:
        448-466): the positive object for cond, then the negative object for uncond, then the SAME negative object for drop-text — each through its own
        check(dit, token, t_mod), as _tea_decide.  Returns (modes, residuals) per branch: 2 + the object's previous_residual for a skip, 1 + the loop's
        residual tensor of that object for a computed step, 0 + None without an object.  A computed decision sets the object's previous_residual to
        the loop's tensor at once — model_fn_wan_talk_video would have stored before the next forward's check —, so a drop-text branch that skips
        right behind a computing uncond branch gets the buffer uncond writes in this very call."""
        t_mod = self.dit.time_mod(timestep)
        B, _, T, H, W = latents.shape
        shape = (B, self.dit.tokens(T, H, W), self.dit.dim)
        modes, residuals = [], []
        for name, cache in (("talk_posi", tea_posi), ("talk_nega", tea_nega), ("talk_nega", tea_nega)):
            if cache is None:
                mode, res = 0, None
            elif cache.check(self.dit, t_mod[:, :1, :1], t_mod):
                mode, res = 2, cache.previous_residual
                if res is None:
                    raise RuntimeError("TeaCache asked to skip before any residual was stored")
            else:
                mode, res = 1, self._tea_residual(name, shape, latents.device)
                cache.previous_residual = res          # what TeaCache.store() would have computed (svi_video.py:64-66), as model_fn_wan_video leaves it
                cache.previous_hidden_states = None
            modes.append(mode)
            residuals.append(res)
        modes = tuple(modes)
        self.talk_tea_counts[modes] = self.talk_tea_counts.get(modes, 0) + 1
        if tea_posi is not None:
            self.tea_counts["skipped" if modes[0] == 2 else "computed"] += 1
        return modes, tuple(residuals)

    def _sample_talk3(self, latents, ctx_pos, ctx_neg, audio_embed_tuple, audio_embed_tuple_null, text_scale, audio_scale, timesteps, step_delta,
                      progress_bar_cmd, cond, tea=None) -> torch.Tensor:
        """The talk clip on the graphed path: both audio tuples are projected into the DiT's audio slots once, then every step is one forward_talk3
        (replayed from the first step's capture) plus the fused three-way guidance + Euler kernel.  `cond`: clip_feature, y, add_condition.  A resident
        loop copies the clip's inputs into its own tensors (adopt) and re-stages the slots where they stand: the next clip of the same shapes replays.
        `tea`: (positive, negative) TeaCache objects, either may be None — the step's three decisions are taken first (_talk_tea_decide), then ONE
        forward_talk3(tea_modes) call runs, replayed from the graph of its mode triple (at most TALK_TEA_GRAPHS alive, the least recently used evicted);
        the two residual tensors are the loop's, slots on a resident loop.  talk_tea_counts counts the clip's steps per triple."""
        ts_dev = timesteps.to(device=latents.device, dtype=torch.float32)
        cond = {k: v for k, v in cond.items() if v is not None}
        # (the talk step's TeaCache is always on the graphed path: a resident loop stays resident with it)
        with self.clip(latents, ctx_pos, ctx_neg, cond, self.resident, every_cond=True, audio_slots=True) as c:
            latents, ctx_pos, ctx_neg, cond = c.latents, c.ctx_pos, c.ctx_neg, c.cond
            if audio_embed_tuple is None and audio_embed_tuple_null is None:      # the caller staged the slots itself (WanDiT.stage_audio_windows)
                if not self.dit.audio_staged(latents.shape[2]):
                    raise ValueError(f"sample_multitalk without audio tuples: the DiT's audio slots are not staged for {latents.shape[2]} latent frames "
                                     "(WanDiT.stage_audio_windows)")
            else:
                self.dit.stage_audio(0, audio_embed_tuple)
                self.dit.stage_audio(1, audio_embed_tuple_null)
            if self._cond is None or self._cond.shape != latents.shape:
                self._cond = torch.empty_like(latents)
                self._uncond = torch.empty_like(latents)
            if self._drop is None or self._drop.shape != latents.shape:
                self._drop = torch.empty_like(latents)
            self.talk_tea_counts = {}
            self.tea_counts = {"computed": 0, "skipped": 0}
            for i, t in enumerate(progress_bar_cmd(timesteps)):
                decided = None if tea is None else self._talk_tea_decide(latents, ts_dev[i:i + 1], tea[0], tea[1])
                self._talk3_graphed(latents, ts_dev[i:i + 1], ctx_pos, ctx_neg, cond, decided)
                ops.cfg3_step_(latents, self._cond, self._uncond, self._drop, text_scale, audio_scale, step_delta(timesteps[i]))
        return c.result()

    @torch.no_grad()
    def sample(self, latents: torch.Tensor, ctx_pos: torch.Tensor, ctx_neg: Optional[torch.Tensor],
               num_inference_steps: int = 50, cfg_scale: float = 5.0, sigma_shift: float = 5.0,
               denoising_strength: float = 1.0, progress_bar_cmd: Callable = lambda x: x, tea_cache_l1_thresh: Optional[float] = None,
               tea_cache_model_id: str = "", cond_wo_pose: bool = False, **cond) -> torch.Tensor:
        """tea_cache_l1_thresh / tea_cache_model_id: as SVIVideoPipeline.__call__ (svi_video.py:442-443, 500-501); None = off.
        add_condition (+ cond_wo_pose): the dance variant's pose embedding, see step()."""
        self.scheduler.set_timesteps(num_inference_steps, denoising_strength=denoising_strength, shift=sigma_shift)
        tea = {}
        if tea_cache_l1_thresh is not None:
            from .teacache import TeaCache
            tea = dict(tea_cache_posi=TeaCache(num_inference_steps, tea_cache_l1_thresh, tea_cache_model_id),
                       tea_cache_nega=TeaCache(num_inference_steps, tea_cache_l1_thresh, tea_cache_model_id))
        ts_dev = self.scheduler.timesteps.to(device=latents.device, dtype=torch.float32)
        self.tea_counts = {"computed": 0, "skipped": 0}
        # the prompt embeddings are constants of the clip: projected (with every block's cross-attention K / V) once, under the context cache
        with self.clip(latents, ctx_pos, ctx_neg, cond, self.stays_resident(bool(tea))) as c:
            for i, t in enumerate(progress_bar_cmd(self.scheduler.timesteps)):
                self.step(c.latents, ts_dev[i:i + 1], self.scheduler.step_delta(t), c.ctx_pos, c.ctx_neg, cfg_scale, cond_wo_pose=cond_wo_pose,
                          **tea, **c.cond)
        return c.result()


# ------------------------------------------------------------------------------------------------------
_INSTALLED: Dict[int, WanDiT] = {}


def _stable_bf16(hip: WanDiT, t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """`t` as contiguous bf16 with a stable address: the conversion of a given tensor (same storage, version, layout) is made once
    and both the original and the copy are kept, so neither address can come back as another prompt's."""
    if t is None or (t.dtype == torch.bfloat16 and t.is_contiguous()):
        return t
    memo = hip.__dict__.setdefault("_bf16_memo", {})
    key = (t.data_ptr(), _version(t), tuple(t.shape), tuple(t.stride()), t.dtype)
    hit = memo.get(key)
    if hit is None:
        if len(memo) >= 8:
            memo.clear()
        hit = memo[key] = (t, t.to(torch.bfloat16).contiguous())
    return hit[1]


def _install_clip(hip: WanDiT) -> dict:
    """How install()'s samplers begin and end a clip (DenoiseLoop.clip): conversions made once per tensor, at a stable address; the context cache
    stays on from clip to clip, as under the swapped model_fn_wan_video."""
    return dict(convert=lambda t: _stable_bf16(hip, t), every_cond=True, keep_cache=True)


def _hip_model_fn(dit_module, x, timestep, context, clip_feature=None, y=None, tea_cache=None, add_condition=None,
                  use_unified_sequence_parallel=False, **kwargs):
    """model_fn_wan_video with the reference's exact signature; `dit_module` is the reference WanModel the
    pipeline still owns (so state_dict()/LoRA loading keep working); its HIP twin is looked up by identity."""
    hip = _INSTALLED.get(id(dit_module))
    if hip is None:
        raise RuntimeError("this WanModel was not passed through svi_hip.install(); refusing to fall back to PyTorch")
    if getattr(dit_module, "vram_management_enabled", False):
        raise RuntimeError("svi_hip: VRAM management was enabled on pipe.dit after install(): the HIP backend reads the parameters in place — install(pipe) again")
    # prompt embeddings are constant across the steps of a clip: the context cache stays on; WanDiT keeps every tensor the cache
    # has seen alive and drops the cache on an in-place write (dit.PromptPins), so a new clip's prompt can never be taken for an
    # old one.  Embeddings that are not bf16-contiguous are converted ONCE per tensor and the copy is what the cache sees.
    if not hip._ctx_cache_on:
        hip.context_cache(True)
    context, clip_feature = _stable_bf16(hip, context), _stable_bf16(hip, clip_feature)
    return model_fn_wan_video(hip, x, timestep, context, clip_feature=clip_feature, y=y, tea_cache=tea_cache,
                              add_condition=add_condition, use_unified_sequence_parallel=use_unified_sequence_parallel)


def _hip_talk_fn(dit_module, x, timestep, context, clip_feature=None, y=None, tea_cache=None, add_condition=None, audio_embed_tuple=None,
                 use_unified_sequence_parallel=False, use_controlnet=False, **kwargs):
    """model_fn_wan_talk_video with the reference's exact signature (pipelines/svi_video_talk.py:83-96), on the HIP twin of `dit_module`."""
    from .dit import model_fn_wan_talk_video
    hip = _INSTALLED.get(id(dit_module))
    if hip is None:
        raise RuntimeError("this WanModel was not passed through svi_hip.install(); refusing to fall back to PyTorch")
    if not hip._ctx_cache_on:
        hip.context_cache(True)
    context, clip_feature = _stable_bf16(hip, context), _stable_bf16(hip, clip_feature)
    return model_fn_wan_talk_video(hip, x, timestep, context, clip_feature=clip_feature, y=y, tea_cache=tea_cache, add_condition=add_condition,
                                   audio_embed_tuple=audio_embed_tuple, use_unified_sequence_parallel=use_unified_sequence_parallel,
                                   use_controlnet=use_controlnet)


def _step_delta_of(scheduler, timestep) -> float:
    """sigma_next - sigma of `scheduler.step(., timestep, .)` for the reference's own FlowMatchScheduler object
    (schedulers/flow_match.py:52-62): the scalar its tensor update multiplies the model output by."""
    if hasattr(scheduler, "step_delta"):
        return scheduler.step_delta(timestep)
    t = timestep.cpu() if isinstance(timestep, torch.Tensor) else timestep
    i = int(torch.argmin((scheduler.timesteps - t).abs()))
    if i + 1 >= len(scheduler.timesteps):
        nxt = 1.0 if (scheduler.inverse_timesteps or scheduler.reverse_sigmas) else 0.0
    else:
        nxt = scheduler.sigmas[i + 1]
    return float(nxt - scheduler.sigmas[i])


def _hip_sample_with_regular_video(self, latents, prompt_emb_posi, prompt_emb_nega, image_emb, extra_input, tea_cache_posi, tea_cache_nega,
                                   usp_kwargs, use_controlnet, cfg_scale, progress_bar_cmd):
    """SVIVideoPipeline._sample_with_regular_video (pipelines/svi_video.py:392-421) with the reference's exact signature, bound onto the
    pipeline by install(): the step loop of the clip on svi_hip.DenoiseLoop — both forwards of a step in one C call (block 0's
    self-attention shared), CFG combine + Euler update in one fused kernel with the reference's bf16 rounding points — i.e. the path
    bench.py times.  Bit-identical to the reference-style loop over the swapped model_fn_wan_video (tests/test_gpu_install.py).
    Anything this loop does not cover (sequence parallelism through usp_kwargs, controlnet, extra inputs, non-bf16 latents) goes to the
    pipeline's original sampler, which still reaches the HIP forward through the swapped module-level model_fn_wan_video."""
    hip = getattr(self, "_svi_hip_dit", None)
    plain = (hip is not None and not extra_input and not use_controlnet and not (usp_kwargs or {}).get("use_unified_sequence_parallel")
             and set(prompt_emb_posi) == {"context"} and set(prompt_emb_nega) == {"context"} and set(image_emb) <= {"clip_feature", "y"}
             and latents.is_cuda and latents.dtype == torch.bfloat16)
    if not plain:
        return self._svi_hip_original_sampler(latents, prompt_emb_posi, prompt_emb_nega, image_emb, extra_input, tea_cache_posi,
                                              tea_cache_nega, usp_kwargs, use_controlnet, cfg_scale, progress_bar_cmd)
    _assert_resident(self, hip, full=True)           # once per clip: offload switched on / parameters moved since install()
    loop = self._svi_hip_loop
    tea = {}
    if (tea_cache_posi or {}).get("tea_cache") is not None:
        tea = dict(tea_cache_posi=tea_cache_posi["tea_cache"], tea_cache_nega=(tea_cache_nega or {}).get("tea_cache"))
    cond = {k: image_emb[k] for k in ("clip_feature", "y") if image_emb.get(k) is not None}
    scale = float(cfg_scale["text"])
    ts_dev = self.scheduler.timesteps.to(device=latents.device, dtype=torch.float32)
    # the rolling window re-enters __call__ per clip (test_svi.py:424-476): a resident loop copies each clip's latents / prompt / conditioning into its
    # own tensors, so clip k+1 replays the step graph clip k captured; the reference's loop leaves its input tensor untouched either way
    with loop.clip(latents, prompt_emb_posi["context"], prompt_emb_nega["context"], cond, loop.stays_resident(bool(tea)), **_install_clip(hip)) as c:
        for progress_id, timestep in enumerate(progress_bar_cmd(self.scheduler.timesteps)):
            loop.step(c.latents, ts_dev[progress_id:progress_id + 1], _step_delta_of(self.scheduler, self.scheduler.timesteps[progress_id]),
                      c.ctx_pos, c.ctx_neg, scale, **tea, **c.cond)
    return c.result()


def _talk_sampler_passes_through(hip, latents, prompt_emb_posi, prompt_emb_nega, image_emb, extra_input, tea_cache_posi, tea_cache_nega, usp_kwargs,
                                 use_controlnet, cfg_scale) -> bool:
    """What install()'s talk sampler hands to the pipeline's original `_sample_with_multitalk` (which still reaches the HIP forward through the swapped
    model_fn_wan_talk_video): TeaCache objects, controlnet, sequence parallelism, extra inputs, prompt / image dicts with other keys than the forward's,
    latents that are not bf16 on the GPU, and the single-forward case (both scales 1)."""
    tea = (tea_cache_posi or {}).get("tea_cache") is not None or (tea_cache_nega or {}).get("tea_cache") is not None
    return bool(hip is None or tea or use_controlnet or (usp_kwargs or {}).get("use_unified_sequence_parallel") or extra_input
                or set(prompt_emb_posi) != {"context"} or set(prompt_emb_nega) != {"context"} or not set(image_emb) <= {"clip_feature", "y"}
                or not getattr(latents, "is_cuda", False) or latents.dtype != torch.bfloat16
                or (cfg_scale["text"] == 1.0 and cfg_scale["audio"] == 1.0))


def _talk_sampler_tea(tea_cache_posi, tea_cache_nega):
    """The (positive, negative) TeaCache objects SVITalkVideoPipeline.__call__ built for a clip (svi_video_talk.py:541-542), or None when neither dict
    carries one."""
    posi, nega = (tea_cache_posi or {}).get("tea_cache"), (tea_cache_nega or {}).get("tea_cache")
    return None if posi is None and nega is None else (posi, nega)


def _talk_sampler_serves_tea(hip, latents, prompt_emb_posi, prompt_emb_nega, image_emb, extra_input, tea_cache_posi, tea_cache_nega, usp_kwargs,
                             use_controlnet, cfg_scale) -> bool:
    """install()'s talk sampler serves a clip with TeaCache objects itself (DenoiseLoop._sample_talk3(tea=...)) when the objects are the ONLY reason
    _talk_sampler_passes_through hands the clip back: that rule, asked with the two TeaCache dicts emptied, must let the clip through.  One object
    in both dicts stays with the pipeline's loop (sample_multitalk says why)."""
    tea = _talk_sampler_tea(tea_cache_posi, tea_cache_nega)
    return bool(tea is not None and tea[0] is not tea[1]
                and not _talk_sampler_passes_through(hip, latents, prompt_emb_posi, prompt_emb_nega, image_emb, extra_input, {}, {}, usp_kwargs,
                                                     use_controlnet, cfg_scale))


def _hip_sample_with_multitalk(self, latents, prompt_emb_posi, prompt_emb_nega, image_emb, extra_input, tea_cache_posi, tea_cache_nega, usp_kwargs,
                               condition, audio_embed_tuple, audio_embed_tuple_null, use_controlnet, cfg_scale, progress_bar_cmd):
    """SVITalkVideoPipeline._sample_with_multitalk (pipelines/svi_video_talk.py:448-466) with the reference's exact signature, bound onto the pipeline by
    install(): the clip's steps on DenoiseLoop's talk path — the three guidance forwards of a step as one captured forward_talk3 call, the audio
    projected once per clip, three-way guidance + Euler update in one fused kernel with the reference's bf16 rounding points.  Bit-identical to the
    reference's loop over the swapped model_fn_wan_talk_video (tests/test_gpu_talk3.py).  What this loop does not cover goes to the pipeline's original
    sampler (_talk_sampler_passes_through) — except a clip whose only reason to go there is a TeaCache object (_talk_sampler_serves_tea): the objects the
    pipeline built drive the loop's one-call step through their own check() and end the clip as the pipeline's loop would have left them
    (previous_residual: the same values, in the loop's tensor)."""
    hip = getattr(self, "_svi_hip_dit", None)
    serves_tea = _talk_sampler_serves_tea(hip, latents, prompt_emb_posi, prompt_emb_nega, image_emb, extra_input, tea_cache_posi, tea_cache_nega,
                                          usp_kwargs, use_controlnet, cfg_scale) and getattr(self, "_svi_hip_loop", None) is not None \
        and self._svi_hip_loop.graph
    if not serves_tea and _talk_sampler_passes_through(hip, latents, prompt_emb_posi, prompt_emb_nega, image_emb, extra_input, tea_cache_posi,
                                                       tea_cache_nega, usp_kwargs, use_controlnet, cfg_scale):
        return self._svi_hip_original_talk_sampler(latents, prompt_emb_posi, prompt_emb_nega, image_emb, extra_input, tea_cache_posi, tea_cache_nega,
                                                   usp_kwargs, condition, audio_embed_tuple, audio_embed_tuple_null, use_controlnet, cfg_scale,
                                                   progress_bar_cmd)
    _assert_resident(self, hip, full=True)           # once per clip: offload switched on / parameters moved since install()
    loop = self._svi_hip_loop
    cond = {k: image_emb[k] for k in ("clip_feature", "y") if image_emb.get(k) is not None}
    if condition is not None:
        cond["add_condition"] = condition
    ctx_p, ctx_n = prompt_emb_posi["context"], prompt_emb_nega["context"]
    if not loop.resident:
        ctx_p, ctx_n = _stable_bf16(hip, ctx_p), _stable_bf16(hip, ctx_n)
    with torch.no_grad():
        return loop._sample_talk3(latents, ctx_p, ctx_n, audio_embed_tuple, audio_embed_tuple_null, float(cfg_scale["text"]), float(cfg_scale["audio"]),
                                  self.scheduler.timesteps, lambda t: _step_delta_of(self.scheduler, t), progress_bar_cmd, cond,
                                  tea=_talk_sampler_tea(tea_cache_posi, tea_cache_nega) if serves_tea else None)


# ------------------------------------------------------------------------------------------------------
# WanVideoPipeline (pipelines/wan_video.py): its step loop is INLINE in __call__ (:266-278), so there is no sampler method to rebind.  Everything around
# the loop — parameter check, scheduler, seeded noise, prompt / image encoding, TeaCache construction, decode, tensor2video (:197-264, :280-290) — must keep
# running as the reference wrote it.  So the reference's own __call__ still runs, whole, and is steered from outside through the seams it already has:
#   * the values the loop needs are picked up where the reference's lines produce them — `self.encode_prompt`, `self.encode_image`,
#     `self.prepare_extra_input(latents)` (the last statement before the loop that sees the initial latents) are shadowed on the instance for the duration
#     of the call by wrappers that call the class's own method and remember what it returned;
#   * `progress_bar_cmd` — called exactly once, with `self.scheduler.timesteps`, to make the loop's iterable (:267) — is replaced by a function that runs
#     the clip's steps on DenoiseLoop (both forwards of a step in one C call, fused CFG + Euler, hipGraph replay; the caller's own progress bar is driven
#     from there) and hands the reference's `for` an EMPTY iterable: its body never runs;
#   * `self.decode_video(latents, ...)` (:281) is shadowed by a wrapper that passes the denoised latents instead of the initial ones.
# Python looks `pipe(...)` up on the TYPE, so the instance gets a subclass of its own class whose __call__ is the steering function (the class itself, and
# other instances, are untouched).  Anything the fast loop does not cover (CPU / non-bf16 latents, extra inputs) passes through: the reference's loop runs
# over the swapped model_fn_wan_video, as install(sampler=False) leaves it.
def _hip_wan_pipeline_call(self, *args, **kwargs):
    import inspect
    cls = type(self).__mro__[1]                      # the pipeline's real class (type(self) is install()'s one-method subclass)
    orig = cls.__call__
    hip = getattr(self, "_svi_hip_dit", None)
    loop = getattr(self, "_svi_hip_loop", None)
    try:
        bound = inspect.signature(orig).bind(self, *args, **kwargs)
        bound.apply_defaults()
        p = bound.arguments
    except TypeError:
        return orig(self, *args, **kwargs)            # let the reference raise its own TypeError
    if hip is None or loop is None or "progress_bar_cmd" not in p:
        return orig(self, *args, **kwargs)
    user_bar = p["progress_bar_cmd"]
    cfg_scale = float(p.get("cfg_scale", 5.0))
    seen = {}

    def remember(name, key_fn=None):
        inner = getattr(cls, name)

        def wrapper(*a, **k):
            out = inner(self, *a, **k)
            seen[key_fn(a, k) if key_fn else name] = out
            if name == "prepare_extra_input":
                seen["latents"] = a[0] if a else k.get("latents")
            return out
        return wrapper

    def steps(timesteps):
        lat, posi, nega, img, extra = seen.get("latents"), seen.get("posi"), seen.get("nega"), seen.get("encode_image") or {}, seen.get("prepare_extra_input")
        plain = (isinstance(lat, torch.Tensor) and lat.is_cuda and lat.dtype == torch.bfloat16 and not extra and isinstance(posi, dict) and set(posi) == {"context"}
                 and (cfg_scale == 1.0 or (isinstance(nega, dict) and set(nega) == {"context"})) and set(img) <= {"clip_feature", "y"}
                 and timesteps is self.scheduler.timesteps)
        if not plain:
            return user_bar(timesteps)                 # the reference's loop, over the swapped model_fn_wan_video
        _assert_resident(self, hip, full=True)
        tea = {}
        if p.get("tea_cache_l1_thresh") is not None:  # as :262-263 builds them: the defining module's own TeaCache, one per branch
            TC = sys.modules[cls.__module__].TeaCache
            mk = lambda: TC(p["num_inference_steps"], rel_l1_thresh=p["tea_cache_l1_thresh"], model_id=p.get("tea_cache_model_id", ""))      # noqa: E731
            tea = dict(tea_cache_posi=mk(), tea_cache_nega=mk())
        cond = {k: img[k] for k in ("clip_feature", "y") if img.get(k) is not None}
        ctx_n = nega["context"] if cfg_scale != 1.0 else None
        # :267 hands the model the timestep in the pipeline's dtype: the bf16-ROUNDED value is what the time embedding sees
        ts_dev = self.scheduler.timesteps.to(dtype=getattr(self, "torch_dtype", torch.float32)).to(device=lat.device, dtype=torch.float32)
        with loop.clip(lat, posi["context"], ctx_n, cond, loop.stays_resident(bool(tea)), **_install_clip(hip)) as c:
            for i, t in enumerate(user_bar(timesteps)):
                loop.step(c.latents, ts_dev[i:i + 1], _step_delta_of(self.scheduler, self.scheduler.timesteps[i]), c.ctx_pos, c.ctx_neg, cfg_scale,
                          **tea, **c.cond)
        seen["denoised"] = c.result()
        return ()

    def decode_video(latents, *a, vae_split=None, vae_group=None, **k):
        # vae_split / vae_group: the exact rank split of the decode (WanVideoVAE.decode); the pipeline's own setting (install(vae_split=...)) unless given
        was = self.__dict__.get("_svi_hip_vae_split")
        if vae_split is not None or vae_group is not None:
            self._svi_hip_vae_split = _vae_split_setting(vae_split, vae_group)
        try:
            return getattr(cls, "decode_video")(self, seen.get("denoised", latents), *a, **k)
        finally:
            self._svi_hip_vae_split = was

    shadows = {"encode_prompt": remember("encode_prompt", lambda a, k: "posi" if (k.get("positive", a[1] if len(a) > 1 else True)) else "nega"),
               "prepare_extra_input": remember("prepare_extra_input"), "decode_video": decode_video}
    if hasattr(cls, "encode_image"):
        shadows["encode_image"] = remember("encode_image")
    p["progress_bar_cmd"] = steps
    for name, fn in shadows.items():
        self.__dict__[name] = fn
    try:
        return orig(*bound.args, **bound.kwargs)
    finally:
        for name in shadows:
            self.__dict__.pop(name, None)


def _vae_split_setting(vae_split, vae_group) -> Optional[dict]:
    """What install()'s VAE decode passes on to WanVideoVAE.decode: nothing (the default: the whole decode on this rank), or split (+ group)."""
    if vae_split is None and vae_group is None:
        return None
    if vae_split is None:
        import torch.distributed as dist
        from .vae import default_vae_split
        vae_split = default_vae_split(dist.get_world_size(vae_group))
    return dict(split=tuple(vae_split), group=vae_group)


def _route_wan_call(pipe, hip) -> bool:
    """install()'s sampler swap for a pipeline whose loop is inline in __call__ (WanVideoPipeline): see _hip_wan_pipeline_call."""
    cls = type(pipe)
    if getattr(cls, "_svi_hip_call_subclass", False):
        cls = cls.__mro__[1]
    need = ("encode_prompt", "prepare_extra_input", "decode_video", "__call__")
    if hasattr(cls, "_sample_with_regular_video") or not all(callable(getattr(cls, n, None)) for n in need):
        return False
    pipe._svi_hip_loop = DenoiseLoop(hip, scheduler=getattr(pipe, "scheduler", None), resident=True)
    sub = type(cls.__name__, (cls,), {"__call__": _hip_wan_pipeline_call, "_svi_hip_call_subclass": True, "__module__": cls.__module__,
                                      "__doc__": cls.__doc__})
    pipe.__class__ = sub
    return True


def _route_dit(pipe, hip, sampler: bool = True) -> None:
    """The swaps of install() that concern the DiT, with the reference's own idioms: the module-level `model_fn_wan_video` (and the talk
    pipeline's `model_fn_wan_talk_video`) of the pipeline's defining module are replaced — every call statement of that module looks the
    name up in the module globals at call time (svi_video.py:401-408) — and, with `sampler`, `_sample_with_regular_video` is rebound on
    the instance with types.MethodType (as svi_video.py:269-271 rebinds `forward` for USP)."""
    dit_module = pipe.dit
    _INSTALLED[id(dit_module)] = hip
    pipe._svi_hip_dit = hip
    mod = sys.modules[type(pipe).__module__]              # (install()'s __call__ subclass keeps the real class's __module__)
    if not hasattr(mod, "_svi_hip_original_model_fn"):
        mod._svi_hip_original_model_fn = getattr(mod, "model_fn_wan_video", None)
    mod.model_fn_wan_video = _hip_model_fn
    if hasattr(mod, "model_fn_wan_talk_video"):        # the talk pipeline's own entry point (pipelines/svi_video_talk.py:83)
        if not hasattr(mod, "_svi_hip_original_talk_fn"):
            mod._svi_hip_original_talk_fn = mod.model_fn_wan_talk_video
        mod.model_fn_wan_talk_video = _hip_talk_fn
    own_sampler = False
    if sampler and hasattr(type(pipe), "_sample_with_regular_video"):
        pipe._svi_hip_original_sampler = types.MethodType(type(pipe)._sample_with_regular_video, pipe)
        pipe._svi_hip_loop = DenoiseLoop(hip, scheduler=getattr(pipe, "scheduler", None), resident=True)
        pipe._sample_with_regular_video = types.MethodType(_hip_sample_with_regular_video, pipe)
        own_sampler = True
    if sampler and hasattr(type(pipe), "_sample_with_multitalk"):      # SVITalkVideoPipeline (svi_video_talk.py:448): the three-forward sampler
        pipe._svi_hip_original_talk_sampler = types.MethodType(type(pipe)._sample_with_multitalk, pipe)
        if not own_sampler:
            pipe._svi_hip_loop = DenoiseLoop(hip, scheduler=getattr(pipe, "scheduler", None), resident=True)
        pipe._sample_with_multitalk = types.MethodType(_hip_sample_with_multitalk, pipe)
        own_sampler = True
    if sampler and not own_sampler:
        _route_wan_call(pipe, hip)                     # WanVideoPipeline: the loop is inline in __call__ (wan_video.py:266-278)


_OFFLOAD_NOTE = ("svi_hip: pipe.{}() is a no-op on an installed pipeline — every model stays resident in HBM (288 GB per MI355X holds the 14B DiT, "
                 "umT5-XXL, CLIP and the VAE together); nothing is wrapped, nothing is offloaded")
_WRAPPERS = ("AutoWrappedModule", "AutoWrappedLinear")        # diffsynth/vram_management/layers.py:12-71


def _unwrap_vram_management(model) -> int:
    """Undo enable_vram_management (vram_management/layers.py:74-94) on one model: an AutoWrappedModule gives its inner module back, an
    AutoWrappedLinear becomes a plain nn.Linear over the same Parameter objects — the state-dict keys are the checkpoint's again.  Returns the
    number of modules restored."""
    n = 0
    for name, child in list(model.named_children()):
        kind = type(child).__name__
        if kind == "AutoWrappedModule" and isinstance(getattr(child, "module", None), torch.nn.Module):
            setattr(model, name, child.module)
            n += 1
        elif kind == "AutoWrappedLinear":
            lin = torch.nn.Linear(child.in_features, child.out_features, bias=child.bias is not None, device="meta")
            lin.weight, lin.bias = child.weight, child.bias
            setattr(model, name, lin)
            n += 1
        else:
            n += _unwrap_vram_management(child)
    if n or getattr(model, "vram_management_enabled", False):
        model.vram_management_enabled = False
    return n


def _neutralise_offload(pipe) -> None:
    """test_svi.py:351 calls pipe.enable_vram_management(num_persistent_param_in_dit=...) unconditionally (and that ends in enable_cpu_offload(),
    svi_video.py:241).  On an installed pipeline both are rebound — the reference's own types.MethodType idiom — to functions that say once
    that they do nothing: the call stays harmless wherever it stands relative to install()."""
    said = pipe.__dict__.setdefault("_svi_hip_said", set())

    def noop(name):
        def f(self, *args, **kwargs):
            if name not in said:
                said.add(name)
                print(_OFFLOAD_NOTE.format(name), file=sys.stderr, flush=True)
        f.__name__ = name
        return f
    for name in ("enable_vram_management", "enable_cpu_offload"):
        if hasattr(pipe, name):
            setattr(pipe, name, types.MethodType(noop(name), pipe))
    if hasattr(pipe, "cpu_offload"):
        pipe.cpu_offload = False


def _make_resident(pipe, device=None) -> None:
    """Everything the clip loop touches, unwrapped and on the GPU: the reference builds its pipeline with only `dit.blocks` on the device
    (svi_video.py:254-256) and relies on load_models_to_device / the VRAM-management wrappers for the rest.  `device`: tests only."""
    dev = torch.device(device or getattr(pipe, "device", None) or "cuda")
    if dev.type != "cuda" and device is None:
        dev = torch.device("cuda")
    for name in ("dit", "vae", "text_encoder", "image_encoder"):
        m = getattr(pipe, name, None)
        if isinstance(m, torch.nn.Module):
            _unwrap_vram_management(m)
            m.to(dev)


def _assert_resident(pipe, hip: WanDiT, full: bool = False) -> None:
    """Refuse loudly when the offload machinery was switched on behind install()'s back (the class's own enable_vram_management called on the
    instance, modules replaced by wrappers, parameters moved off the device): the HIP side borrows parameter storage by pointer and would
    otherwise keep computing on stale, kept-alive copies.  `full`: walk every parameter (once per clip); otherwise flags only (every forward)."""
    dit_module = getattr(pipe, "dit", None)
    if getattr(pipe, "cpu_offload", False) or getattr(dit_module, "vram_management_enabled", False):
        raise RuntimeError("svi_hip: CPU offload / VRAM management was enabled on an installed pipeline (pipe.cpu_offload or pipe.dit.vram_management_enabled is set): "
                           "the HIP backend keeps every model resident and reads the DiT's parameters in place — call svi_hip.install(pipe) again to restore residency")
    if full and dit_module is not None:
        hip.check_module_in_place(dit_module)


def install(pipe, vae: bool = True, encoders: bool = True, sampler: bool = True, resident: bool = True, vae_split=None, vae_group=None,
            vae_encode_split=None, fp8_resident=None):
    """Route `pipe`'s hot path (SVIVideoPipeline / WanVideoPipeline of the reference) through libsvi_hip.

    * `model_fn_wan_video` in the pipeline's defining module is replaced by the HIP-backed function
      (every call site in that module — the cond/uncond forwards of the sampler — picks it up);
    * with `sampler`: `pipe._sample_with_regular_video` (svi_video.py:392-421) is rebound to the DenoiseLoop-backed sampler of the same
      signature — one C call for the two forwards of a step, fused CFG + Euler kernel: the loop bench.py times; a WanVideoPipeline, whose loop is
      inline in `__call__` (wan_video.py:266-278), gets the same loop through `_hip_wan_pipeline_call` (the reference's own `__call__` keeps running
      around it: every line outside the loop is the reference's); an SVITalkVideoPipeline's `_sample_with_multitalk` (svi_video_talk.py:448-466) is
      rebound to `_hip_sample_with_multitalk` — the three guidance forwards of a step as one captured call, the audio projected once per clip;
    * `pipe.vae.encode/decode` are rebound to the HIP VAE (same signatures), when `vae` is true; `vae_split` = (parts_h, parts_w) (+ `vae_group`, whose
      ranks each decode one part; a group alone takes default_vae_split's grid) makes every decode the exact spatial split of WanVideoVAE.decode —
      off by default; call the pipeline with tiled=False then, the blended tiling and the split exclude each other; `vae_encode_split` (a grid, or
      True for default_vae_split's grid over `vae_group`) does the same for every encode (WanVideoVAE.encode), independent of `vae_split`, off by default;
    * `pipe.dit` stays the reference nn.Module: weights are borrowed, so call `install` again (or
      `pipe._svi_hip_dit.rebind()`) after `load_lora_v2`, `.to()` or any offload that moves storage.
    * with `encoders`: the prompter's `text_encoder(ids, mask)` (prompters/wan_prompter.py:109) and `pipe.image_encoder.encode_image`
      (svi_video.py:317) go to the HIP encoders when those modules are on the GPU (text encoder in bf16; the image encoder's
      parameters are copied to fp32, the precision SVI switches that module to around the call, :307-309).
    * with `resident` (default): the pipeline's models are made resident first — VRAM-management wrappers undone (AutoWrappedLinear /
      AutoWrappedModule, vram_management/layers.py), every model moved to pipe.device — and `pipe.enable_vram_management` /
      `pipe.enable_cpu_offload` are rebound to no-ops that say so once: test_svi.py:316-351 runs unchanged with `svi_hip.install(pipe)` added
      before OR after its line 351.  288 GB of HBM holds every model; nothing is offloaded.  If offload is switched on behind install()'s back
      (the class's function called on the instance, a module moved to the CPU) the next clip refuses with a RuntimeError instead of computing
      on stale copies; parameters that merely moved on the device (a LoRA merge that re-created them) are re-bound.
    * `fp8_resident` (default: False, or SVI_FP8_RESIDENT): a DiT whose parameters are float8_e4m3fn (test_svi.py:337) keeps its blocks' Linear weights as the
      stored bytes — no bf16 copies (WanDiT.bind); the same bits, a third of the memory.
    """
    if resident:
        _make_resident(pipe)
        _neutralise_offload(pipe)
    dit_module = pipe.dit
    wrapped = [n for n, m in dit_module.named_modules() if type(m).__name__ in _WRAPPERS]
    if wrapped:
        raise RuntimeError(f"install(): pipe.dit still holds VRAM-management wrappers ({wrapped[0]} ...): call install(pipe) with resident=True, or before "
                           "pipe.enable_vram_management()")
    off = [n for n, p in dit_module.named_parameters() if not p.is_cuda or p.dtype not in (torch.bfloat16, torch.float8_e4m3fn)]
    if off:
        raise RuntimeError(f"install(): the DiT must be on the GPU in bf16 (or FP8 storage) — {off[0]} is {dict(dit_module.named_parameters())[off[0]].device}/"
                           f"{dict(dit_module.named_parameters())[off[0]].dtype}; pipe.dit.to('cuda', torch.bfloat16) first, or install(pipe, resident=True)")
    hip = WanDiT.from_module(dit_module, fp8_resident=fp8_resident)
    _route_dit(pipe, hip, sampler=sampler)
    if vae and getattr(pipe, "vae", None) is not None:
        from .vae import WanVideoVAE, _encode_split_setting
        hv = WanVideoVAE.from_module(pipe.vae)
        pipe._svi_hip_vae = hv
        enc_split = _encode_split_setting(vae_encode_split, vae_group)
        pipe.vae.encode = types.MethodType(lambda self, videos, device=None, tiled=False, tile_size=(34, 34),
                                           tile_stride=(18, 16): hv.encode(videos, device, tiled, tile_size, tile_stride, **enc_split), pipe.vae)
        pipe._svi_hip_vae_split = _vae_split_setting(vae_split, vae_group)
        pipe.vae.decode = types.MethodType(lambda self, hidden_states, device=None, tiled=False, tile_size=(34, 34),
                                           tile_stride=(18, 16): hv.decode(hidden_states, device, tiled, tile_size, tile_stride,
                                                                           **(pipe.__dict__.get("_svi_hip_vae_split") or {})), pipe.vae)
    if encoders:
        from .encoders import WanImageEncoder, WanTextEncoder
        te = getattr(pipe, "text_encoder", None)
        prompter = getattr(pipe, "prompter", None)
        if te is not None and prompter is not None:
            q = next(te.parameters())
            if q.is_cuda and q.dtype == torch.bfloat16:
                pipe._svi_hip_text_encoder = ht = WanTextEncoder.from_module(te)
                # encode_prompt zeroes the padded rows right after the call (:110-111): compute the valid ones only
                prompter.text_encoder = lambda ids, mask=None: ht.forward(ids, mask, rows="valid")
        ie = getattr(pipe, "image_encoder", None)
        if ie is not None and next(ie.parameters()).is_cuda:
            pipe._svi_hip_image_encoder = hi = WanImageEncoder.from_module(ie)
            ie.encode_image = types.MethodType(lambda self, videos: hi.encode_image(videos), ie)
    return pipe
