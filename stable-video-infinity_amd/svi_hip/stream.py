"""The clip loop of an image-conditioned stream (test_svi.py:424-476 around SVIVideoPipeline.__call__), resident on the GPU.

Per clip the reference: encodes the motion frames (the last `num_motion_frames` 8-bit frames of the previous clip, or the input
image) plus padding with the VAE into y (encode_images_adaptive, svi_video.py:291-364), denoises 50 steps, decodes, converts the
video to 8-bit PIL frames (tensor2video :366-370), keeps all but the last `num_motion_frames` of them (test_svi.py:472-476) and hands
those last frames — as 8-bit images, through preprocess_image — to the next clip.  Here the same sequence runs without leaving
HBM: the 8-bit quantisation and its inverse are device kernels with the reference's fp32 arithmetic (svi_video_to_u8 /
svi_u8_to_video), so the frames and the next clip's conditioning are what the host round trip would give.

Outside SURVEY §8's path and therefore injected: the prompt embeddings (T5) and the CLIP image feature of each clip's first frame
(`clip_encoder`, a callable [1, 3, H, W] float in [-1, 1] -> [1, 257, 1280]).
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Callable, List, Optional, Sequence

import torch

from . import _lib as L
from .conditioning import image_condition
from .pipeline import DenoiseLoop, generate_noise
from .vae import _encode_split_setting, default_vae_split, latency_group


def video_to_u8(video: torch.Tensor) -> torch.Tensor:
    """video fp32 [3, T, H, W] in [-1, 1] -> 8-bit frames [T, H, W, 3]   (tensor2video, svi_video.py:366-370)."""
    video = video.to(device="cuda", dtype=torch.float32).contiguous()
    _, T, H, W = video.shape
    out = torch.empty((T, H, W, 3), dtype=torch.uint8, device=video.device)
    L.check(L.lib().svi_video_to_u8(L.ptr(video), L.ptr(out), T, H, W, L.current_stream()), "svi_video_to_u8")
    return out


def u8_to_video(frames: torch.Tensor) -> torch.Tensor:
    """8-bit frames [n, H, W, 3] -> fp32 [n, 3, H, W] = x * (2 / 255) - 1   (preprocess_image, pipelines/base.py:44-45)."""
    frames = frames.to(device="cuda", dtype=torch.uint8).contiguous()
    n, H, W, _ = frames.shape
    out = torch.empty((n, 3, H, W), dtype=torch.float32, device=frames.device)
    L.check(L.lib().svi_u8_to_video(L.ptr(frames), L.ptr(out), n, H, W, L.current_stream()), "svi_u8_to_video")
    return out


def seeds_per_clip(seed, num_clips: int) -> List[int]:
    """`seed` — one int for every clip, or one per clip — as the list of the clips' seeds."""
    seeds = [int(seed)] * num_clips if isinstance(seed, int) else [int(s) for s in seed]
    if len(seeds) != num_clips:
        raise ValueError(f"{len(seeds)} seeds for {num_clips} clips")
    return seeds


class StreamLoop:
    """The one clip walk (_walk).  A variant says what differs: the single-rank DenoiseLoop it runs on (`single_rank`), what clip k is sampled
    with (_clip_inputs), which sampler runs (_sample), what the trace notes of the loop afterwards (_loop_trace), and whether a clip is stitched
    whole (`stitch_whole`) or loses the motion frames it hands on."""
    single_rank = dict(resident=True)      # every clip of the stream replays the step graph the first one captured
    stitch_whole = False

    def __init__(self, dit, vae, clip_encoder: Optional[Callable[[torch.Tensor], torch.Tensor]] = None, num_motion_frames: int = 1,
                 num_frames: int = 81, num_inference_steps: int = 50, cfg_scale: float = 5.0, sigma_shift: float = 5.0,
                 ref_pad_cfg: bool = False, ref_pad_num: int = 0, seed_times: int = 42, tiled: bool = False, tile_size=(30, 52),
                 tile_stride=(15, 26), vae_split=None, vae_group=None, cfg_pair=None, sp_group=None, sequence_parallel: bool = False,
                 vae_encode_split=None):
        """tiled / tile_size / tile_stride: the VAE tiling arguments SVIVideoPipeline.__call__ passes to decode_video (svi_video.py:439-441, 515;
        test_svi.py passes args.tiled, default False).  The conditioning encode is never tiled, as in the reference (:350).
        vae_split = (parts_h, parts_w) / vae_group: the exact spatial split of every clip's decode (WanVideoVAE.decode): with a group each rank
        decodes one part, without one all parts run here, one after another.  Off by default.  cfg_pair / sequence_parallel (+ sp_group): the
        latency modes of DenoiseLoop; the decode then uses that group's ranks too, on default_vae_split's grid unless vae_split names one.
        vae_encode_split: the same split for every clip's conditioning encode (WanVideoVAE.encode), independent of vae_split and off by default
        (None / False), in the latency modes too.  (parts_h, parts_w): that grid, over vae_group (else the latency group) when there is one, all
        parts here otherwise.  True: default_vae_split's grid over that group; without a group there is nothing to split over."""
        if num_motion_frames < 1:
            raise ValueError("an image-conditioned stream hands at least one motion frame from clip to clip (test_svi.py:472-476)")
        enc_group = vae_group
        if cfg_pair is not None or sequence_parallel:
            self.loop = DenoiseLoop(dit, cfg_pair=cfg_pair, sp_group=sp_group, sequence_parallel=sequence_parallel)
            if enc_group is None:
                enc_group = latency_group(self.loop)
            if vae_group is None and (vae_split is None or tuple(vae_split) != (1, 1)):
                vae_group = latency_group(self.loop)
        else:
            self.loop = DenoiseLoop(dit, **self.single_rank)
        if vae_group is not None and vae_split is None:
            import torch.distributed as dist
            vae_split = default_vae_split(dist.get_world_size(vae_group))
        if vae_split is not None and tiled:
            raise ValueError("StreamLoop: tiled=True blends overlapping tiles, vae_split is the exact rank split; ask for one of them")
        self.vae_split = dict(split=tuple(vae_split), group=vae_group) if vae_split is not None else {}
        self.vae_encode_split = _encode_split_setting(vae_encode_split, enc_group)
        self.vae, self.clip_encoder = vae, clip_encoder
        self.num_motion_frames, self.num_frames = num_motion_frames, num_frames
        self.steps, self.cfg_scale, self.sigma_shift = num_inference_steps, cfg_scale, sigma_shift
        self.ref_pad_cfg, self.ref_pad_num, self.seed_times = ref_pad_cfg, ref_pad_num, seed_times
        self.tiler = dict(tiled=tiled, tile_size=tuple(tile_size), tile_stride=tuple(tile_stride))
        self.trace: List[dict] = []                     # per clip: what conditioned it (for tests / inspection)

    @torch.no_grad()
    def run(self, input_frames_u8: torch.Tensor, ref_frame_u8: torch.Tensor, prompts: Sequence[tuple], num_clips: int,
            prompt_repeat_times: int = 1, use_first_prompt_only: bool = False, clip_feature: Optional[torch.Tensor] = None,
            start_clip: int = 0) -> torch.Tensor:
        """input_frames_u8 [n, H, W, 3] (the input image, n = 1, or the motion frames of an earlier stream), ref_frame_u8 [H, W, 3]
        (`random_ref_frame`), prompts: list of (context_pos, context_neg) embeddings.  Returns the stitched 8-bit video
        [frames, H, W, 3] on the GPU: every clip but the last loses its final `num_motion_frames` frames.
        `start_clip`: resume a stream at clip index k (input_frames_u8 = the motion frames clip k-1 handed over): clips
        k .. num_clips-1 run with the seeds and prompts of their own indices."""
        return self._walk(range(start_clip, num_clips), num_clips, input_frames_u8, ref_frame_u8, clip_feature,
                          SimpleNamespace(prompts=prompts, prompt_repeat_times=prompt_repeat_times, use_first_prompt_only=use_first_prompt_only))

    def _clip_feature(self, first: torch.Tensor, clip_feature: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        """The CLIP feature of a clip's first motion frame, or the caller's when the loop has no encoder."""
        if self.clip_encoder is None:
            return clip_feature
        if hasattr(self.clip_encoder, "encode_image"):                            # svi_hip.WanImageEncoder: clip_context of svi_video.py:317, :355
            return self.clip_encoder.encode_image([first[:1]]).to(torch.bfloat16)
        return self.clip_encoder(first[:1])

    def _clip_inputs(self, k: int, run):
        """What clip k is sampled with: (seed, (ctx_pos, ctx_neg), further keywords of the sampler — conditions —, further trace entries).  `run`:
        what run() handed to _walk, plus the clip's tlat, H and W.  Called at the clip boundary, behind the conditioning encode."""
        from .parallel import clip_prompt_index, clip_seed
        prompt = run.prompts[clip_prompt_index(k, len(run.prompts), run.prompt_repeat_times, run.use_first_prompt_only)]
        return clip_seed(k, self.seed_times), prompt, {}, {}

    def _sample(self, lat, ctx_pos, ctx_neg, cond) -> torch.Tensor:
        return self.loop.sample(lat, ctx_pos, ctx_neg, num_inference_steps=self.steps, cfg_scale=self.cfg_scale, sigma_shift=self.sigma_shift, **cond)

    def _loop_trace(self) -> dict:
        """Trace entries read off the loop once a clip is sampled."""
        return {}

    def _walk(self, clips, num_clips: int, input_frames_u8, ref_frame_u8, clip_feature, run) -> torch.Tensor:
        """Clips `clips` of a stream of `num_clips`, stitched.  The model is handed back as it came, whatever ends the walk."""
        motion = input_frames_u8.to("cuda")
        ref = u8_to_video(ref_frame_u8.to("cuda")[None])[0]
        run.H, run.W = H, W = motion.shape[1:3]
        run.tlat = tlat = (self.num_frames - 1) // 4 + 1
        pieces = []
        self.trace = []
        cache_was_on = self.loop.dit._ctx_cache_on
        try:
            for k in clips:
                first = u8_to_video(motion)                                          # preprocess_image of every motion frame
                y = image_condition(self.vae, first, ref, self.num_frames, self.ref_pad_cfg, self.ref_pad_num, **self.vae_encode_split)
                cond = dict(y=y)
                cf = self._clip_feature(first, clip_feature)
                if cf is not None:
                    cond["clip_feature"] = cf
                seed, (ctx_pos, ctx_neg), more, noted = self._clip_inputs(k, run)
                lat = generate_noise((1, 16, tlat, H // 8, W // 8), seed=seed, device="cpu", dtype=torch.float32).to("cuda", torch.bfloat16)
                lat = self._sample(lat, ctx_pos, ctx_neg, dict(cond, **more))
                video = self.vae.decode(lat.float(), device="cuda", **self.tiler, **self.vae_split)[0]  # [3, num_frames, H, W] fp32
                frames = video_to_u8(video)
                self.trace.append(dict(clip=k, seed=seed, motion=motion, y=y, latents=lat, frames=frames, **noted, **self._loop_trace()))
                motion = frames[-self.num_motion_frames:]
                pieces.append(frames if self.stitch_whole or k == num_clips - 1 else frames[:-self.num_motion_frames])
        finally:
            if not cache_was_on:
                self.loop.close()      # the resident loop keeps the context cache on from clip to clip; hand the model back as it came
        return torch.cat(pieces, dim=0)


class TalkStreamLoop(StreamLoop):
    """The clip loop of a talk stream (test_svi_talk.py:277-302 around SVITalkVideoPipeline.__call__, svi_video_talk.py:469-564), resident on the GPU.

    Per clip the reference: cuts the clip's audio windows out of the whole file's wav2vec2 embedding at `audio_start_idx` (get_audio_embedding +
    preprocess_audio, a host gather, six rearrange / concat passes and an upload), encodes the motion frames — the last `num_motion_frames` 8-bit
    frames of the previous clip, or the input image — plus padding into y, denoises with the three-way guidance (_sample_with_multitalk), decodes,
    converts to 8-bit frames and appends ALL of them to the video (`video_list += video`: clips are stitched whole).  Here the embedding [N, 12, 768]
    is uploaded once; at a clip boundary both audio slots of the DiT are cut and re-projected on the device where they stand
    (WanDiT.stage_audio_windows), so every clip after the first replays the first clip's step graph(s) on ONE DenoiseLoop(graph=True, resident=True);
    the motion frames go through StreamLoop's 8-bit hand-off.  The audio encoder runs once per audio file: its output is this loop's input, or
    the loop runs it itself on the device (run(speech=, audio_encoder=), svi_hip.WanAudioEncoder).  Clips chain, so there is no clip-per-rank mode; under a CFG pair the talk step's three forwards have no home and it is refused.
    With sequence_parallel the loop keeps DenoiseLoop's eager shard forwards (the windows are cut on the device all the same, ops.audio_windows)."""
    single_rank = dict(graph=True, resident=True)
    stitch_whole = True                         # `video_list += video` in both branches of test_svi_talk.py:304-308: every clip whole

    def __init__(self, dit, vae, clip_encoder: Optional[Callable[[torch.Tensor], torch.Tensor]] = None, num_motion_frames: int = 1,
                 num_frames: int = 81, num_inference_steps: int = 50, cfg_scale: Optional[dict] = None, sigma_shift: float = 5.0,
                 ref_pad_cfg: bool = False, ref_pad_num: int = 0, tea_cache_l1_thresh: Optional[float] = None, tea_cache_model_id: str = "",
                 tiled: bool = False, tile_size=(30, 52), tile_stride=(15, 26), vae_split=None, vae_group=None, cfg_pair=None, sp_group=None,
                 sequence_parallel: bool = False, vae_encode_split=None):
        """cfg_scale = dict(audio=, text=) (test_svi_talk.py:287-289; default audio 4, text 5).  tea_cache_l1_thresh / tea_cache_model_id: TeaCache with
        fresh objects per clip, as SVITalkVideoPipeline.__call__ makes them (svi_video_talk.py:541-542).  Everything else as StreamLoop."""
        if cfg_pair is not None:
            raise ValueError("TalkStreamLoop: the talk step has three guidance forwards whose branches differ in their audio; a CFG-pair rank serves two "
                             "(use sequence_parallel, or one rank)")
        if not getattr(dit, "enable_multitalk", False):
            raise ValueError("TalkStreamLoop needs a DiT with enable_multitalk")
        if num_frames % 4 != 1:
            raise ValueError(f"num_frames must be 4 k + 1 (got {num_frames}; the reference rounds it up before it cuts the audio, svi_video_talk.py:499-501)")
        cfg_scale = dict(cfg_scale or dict(audio=4.0, text=5.0))
        if set(cfg_scale) != {"audio", "text"}:
            raise ValueError(f"cfg_scale must be dict(audio=, text=) (got {cfg_scale!r})")
        super().__init__(dit, vae, clip_encoder=clip_encoder, num_motion_frames=num_motion_frames, num_frames=num_frames,
                         num_inference_steps=num_inference_steps, cfg_scale=cfg_scale, sigma_shift=sigma_shift, ref_pad_cfg=ref_pad_cfg,
                         ref_pad_num=ref_pad_num, tiled=tiled, tile_size=tile_size, tile_stride=tile_stride, vae_split=vae_split, vae_group=vae_group,
                         sp_group=sp_group, sequence_parallel=sequence_parallel, vae_encode_split=vae_encode_split)
        self.tea = dict(tea_cache_l1_thresh=tea_cache_l1_thresh, tea_cache_model_id=tea_cache_model_id)

    def audio_start(self, k: int) -> int:
        """Clip k's audio_start_idx: k clips' worth of frames, minus the motion frames every clip after the first re-renders (test_svi_talk.py:278-280,
        with the clip's own frame count in the place of the script's 81)."""
        return k * self.num_frames - (self.num_motion_frames if k > 0 else 0)

    @torch.no_grad()
    def run(self, input_frames_u8: torch.Tensor, ref_frame_u8: torch.Tensor, prompt: tuple, audio_emb: Optional[torch.Tensor] = None,
            num_clips: Optional[int] = None, seed=0, clip_feature: Optional[torch.Tensor] = None, null_emb: Optional[torch.Tensor] = None, *,
            speech=None, audio_encoder=None, audio_embedding: Optional[torch.Tensor] = None) -> torch.Tensor:
        """input_frames_u8 [n, H, W, 3] (the input image, n = 1), ref_frame_u8 [H, W, 3] (`random_ref_frame`, fixed for the stream), prompt =
        (context_pos, context_neg) embeddings, audio_emb (or audio_embedding=) fp32 or bf16 [N, 12, 768]: the audio encoder's output for the whole
        stream (a stream that outlasts it keeps reading its last row: the reference's clamp).  Instead of the embedding: speech= the loudness-normalised
        16 kHz mono samples (1-D tensor or ndarray) and audio_encoder= an svi_hip.WanAudioEncoder — encoded once per stream on the device
        (get_embedding, utils/audio_process.py:18-41), the result never leaves HBM.  seed: one int for every clip (the reference's call) or one per
        clip.  null_emb: WanDiT.stage_audio_windows's.  Returns the stitched 8-bit video [num_clips * num_frames, H, W, 3] on the GPU: every clip whole."""
        if num_clips is None:
            raise TypeError("TalkStreamLoop.run: num_clips is required")
        if audio_embedding is not None:
            if audio_emb is not None:
                raise TypeError("TalkStreamLoop.run: audio_emb and audio_embedding name the same argument")
            audio_emb = audio_embedding
        if (speech is None) == (audio_emb is None):
            raise TypeError("TalkStreamLoop.run: pass either the audio embedding or speech= with audio_encoder=")
        if speech is not None:
            if audio_encoder is None:
                raise TypeError("TalkStreamLoop.run: speech= needs audio_encoder= (an svi_hip.WanAudioEncoder)")
            audio_emb = audio_encoder.encode(speech)
        seeds = seeds_per_clip(seed, num_clips)
        if audio_emb.dim() != 3 or tuple(audio_emb.shape[1:]) != (12, 768) or audio_emb.shape[0] < 1:
            raise ValueError(f"audio_emb must be [N >= 1, 12, 768] (got {tuple(audio_emb.shape)})")
        emb = audio_emb.to("cuda")
        emb = (emb if emb.dtype in (torch.float32, torch.bfloat16) else emb.float()).contiguous()
        if null_emb is not None:
            null_emb = null_emb.to("cuda").contiguous()
        slots = self.loop.graph and any(s != 1.0 for s in self._scales().values())      # sample_multitalk's one-call step reads the slots
        return self._walk(range(num_clips), num_clips, input_frames_u8, ref_frame_u8, clip_feature,
                          SimpleNamespace(seeds=seeds, prompt=prompt, emb=emb, null_emb=null_emb, slots=slots))

    def _scales(self) -> dict:
        return dict(text_scale=float(self.cfg_scale["text"]), audio_scale=float(self.cfg_scale["audio"]))

    def _clip_inputs(self, k: int, run):
        start = self.audio_start(k)
        if run.slots:
            self.loop.dit.stage_audio_windows(run.emb, start, run.tlat, run.null_emb)
            aud = aud0 = None
        else:
            aud, aud0 = self._tuples(run.emb, start, run.tlat), self._tuples(run.null_emb, start, run.tlat)
        return run.seeds[k], run.prompt, dict(audio_embed_tuple=aud, audio_embed_tuple_null=aud0), dict(audio_start=start)

    def _sample(self, lat, ctx_pos, ctx_neg, cond) -> torch.Tensor:
        return self.loop.sample_multitalk(lat, ctx_pos, ctx_neg, num_inference_steps=self.steps, sigma_shift=self.sigma_shift, **self._scales(),
                                          **self.tea, **cond)

    def _loop_trace(self) -> dict:
        return dict(captures=self.loop.captures, graphs=self.loop.held_graphs(), generation=self.loop.dit.generation())

    @staticmethod
    def _tuples(emb: Optional[torch.Tensor], start: int, tlat: int):
        """audio_embed_tuple for the eager forwards, cut on the device; None: the reference's null audio (zeros, svi_video_talk.py:550)."""
        from .ops import audio_windows
        if emb is None:
            emb = torch.zeros((1, 12, 768), dtype=torch.bfloat16, device="cuda")
        first, latter = audio_windows(emb, start, tlat)
        return first[None], latter[None]


class DanceStreamLoop(StreamLoop):
    """The clip loop of a dance stream (test_svi_dance.py:238-288 around SVIDanceVideoPipeline.__call__, svi_video_dance.py:447-546), resident on the GPU.

    Between two clips the reference's script builds the next pose window on the host — the last `num_motion_frames` poses of the previous window, the
    rest read on from the whole pose video at a cursor that wraps; every frame resized with nearest-neighbour and padded to the centre; converted to
    float and uploaded (3 F H W fp32 values) — and the pipeline embeds it (dwpose_embedding, :527-530) into the `add_condition` of both guidance
    forwards (`cond_wo_pose`) or of the conditional one alone.  Here the pose video is uploaded once, as the 8-bit frames [N, h, w, 3] the video reader
    hands over; a clip boundary is one window launch with scalar arguments (PoseEmbedder.window) and the embedder, and every clip after the first
    replays the first clip's step graph on ONE DenoiseLoop(resident=True), which copies the condition into the tensor it owns.  The motion frames go
    through StreamLoop's 8-bit hand-off, the video is stitched by StreamLoop's rule (every clip but the last loses its final motion frames, :262-267).
    The dance pipeline's encode_images_adaptive is the plain one, line for line (svi_video_dance.py:314-387 / svi_video.py:291-364): image_condition."""

    def __init__(self, dit, vae, pose_embedder, clip_encoder: Optional[Callable[[torch.Tensor], torch.Tensor]] = None, num_motion_frames: int = 1,
                 num_frames: int = 81, num_inference_steps: int = 50, cfg_scale: Optional[dict] = None, sigma_shift: float = 5.0,
                 cond_wo_pose: bool = True, remove_pose: bool = False, ref_pad_cfg: bool = False, ref_pad_num: int = 0,
                 tea_cache_l1_thresh: Optional[float] = None, tea_cache_model_id: str = "", tiled: bool = False, tile_size=(30, 52),
                 tile_stride=(15, 26), vae_split=None, vae_group=None, cfg_pair=None, sp_group=None, sequence_parallel: bool = False,
                 vae_encode_split=None):
        """pose_embedder: an svi_hip.PoseEmbedder of the DiT's width.  cfg_scale = dict(audio=, text=) as the script passes it (test_svi_dance.py:248-250);
        the sampler reads 'text' only (svi_video_dance.py:421-433).  cond_wo_pose: the pose condition also on the unconditional forward — True is what the
        script passes (:259).  remove_pose: the script's --remove_pose, no pose condition at all (:252).  tea_cache_l1_thresh / tea_cache_model_id: TeaCache
        with fresh objects per clip, as SVIDanceVideoPipeline.__call__ makes them (svi_video_dance.py:519-520).  Everything else as StreamLoop."""
        if num_frames % 4 != 1:
            raise ValueError(f"num_frames must be 4 k + 1 (got {num_frames}; the pose window and the latents are cut for the same frame count)")
        if num_motion_frames < 1 or num_motion_frames >= num_frames:
            raise ValueError(f"num_motion_frames must be in 1 .. num_frames - 1 = {num_frames - 1} (got {num_motion_frames}): the pose window carries "
                             "them over and reads on")
        cfg_scale = dict(cfg_scale or dict(audio=4.0, text=5.0))
        if "text" not in cfg_scale:
            raise ValueError(f"cfg_scale must be a dict with 'text' (got {cfg_scale!r})")
        if pose_embedder.dim != dit.dim:
            raise ValueError(f"the pose embedder's dim {pose_embedder.dim} is not the DiT's dim {dit.dim}")
        super().__init__(dit, vae, clip_encoder=clip_encoder, num_motion_frames=num_motion_frames, num_frames=num_frames,
                         num_inference_steps=num_inference_steps, cfg_scale=cfg_scale, sigma_shift=sigma_shift, ref_pad_cfg=ref_pad_cfg,
                         ref_pad_num=ref_pad_num, tiled=tiled, tile_size=tile_size, tile_stride=tile_stride, vae_split=vae_split, vae_group=vae_group,
                         cfg_pair=cfg_pair, sp_group=sp_group, sequence_parallel=sequence_parallel, vae_encode_split=vae_encode_split)
        self.pose_embedder, self.cond_wo_pose, self.remove_pose = pose_embedder, bool(cond_wo_pose), bool(remove_pose)
        self.tea = dict(tea_cache_l1_thresh=tea_cache_l1_thresh, tea_cache_model_id=tea_cache_model_id)

    @torch.no_grad()
    def run(self, input_frames_u8: torch.Tensor, ref_frame_u8: torch.Tensor, prompt: tuple, pose_u8: torch.Tensor, num_clips: int, seed=0,
            clip_feature: Optional[torch.Tensor] = None) -> torch.Tensor:
        """input_frames_u8 [n, H, W, 3] (the reference image at the clip size, n = 1), ref_frame_u8 [H, W, 3] (`random_ref_frame`, fixed for the stream),
        prompt = (context_pos, context_neg) embeddings, pose_u8 uint8 [N, h, w, 3]: the whole pose video at its source resolution (a stream that
        outlasts it wraps around; one shorter than a clip repeats).  seed: one int for every clip or one per clip (the script passes None: random).
        Returns the stitched 8-bit video on the GPU: every clip but the last loses its final `num_motion_frames` frames."""
        seeds = seeds_per_clip(seed, num_clips)
        if pose_u8.dtype != torch.uint8 or pose_u8.dim() != 4 or pose_u8.shape[0] < 1 or pose_u8.shape[3] != 3:
            raise ValueError(f"pose_u8 must be uint8 [N >= 1, h, w, 3] (got {pose_u8.dtype}, {tuple(pose_u8.shape)})")
        H, W = input_frames_u8.shape[1:3]
        tlat = (self.num_frames - 1) // 4 + 1
        pt, ph, pw = self.loop.dit.patch_size
        grid, pose_grid = (tlat // pt, H // 8 // ph, W // 8 // pw), self.pose_embedder.tokens(self.num_frames, H, W)
        if pose_grid != grid:
            raise ValueError(f"the pose embedder's token grid {pose_grid} for {self.num_frames} frames of {H} x {W} is not the DiT's {grid} for the clip's latents")
        pose = pose_u8.to("cuda").contiguous()                   # once per stream
        return self._walk(range(num_clips), num_clips, input_frames_u8, ref_frame_u8, clip_feature, SimpleNamespace(seeds=seeds, prompt=prompt, pose=pose))

    def _clip_inputs(self, k: int, run):
        if self.remove_pose:
            return run.seeds[k], run.prompt, {}, dict(pose_window=None, add_condition=None)
        window = self.pose_embedder.window(run.pose, k, self.num_frames, self.num_motion_frames, run.H, run.W)
        return run.seeds[k], run.prompt, dict(add_condition=window), dict(pose_window=k, add_condition=window)

    def _sample(self, lat, ctx_pos, ctx_neg, cond) -> torch.Tensor:
        return self.loop.sample(lat, ctx_pos, ctx_neg, num_inference_steps=self.steps, cfg_scale=float(self.cfg_scale["text"]),
                                sigma_shift=self.sigma_shift, cond_wo_pose=self.cond_wo_pose, **self.tea, **cond)

    def _loop_trace(self) -> dict:
        return dict(captures=self.loop.captures, graphs=self.loop.held_graphs())
