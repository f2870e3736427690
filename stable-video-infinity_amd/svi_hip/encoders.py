"""Prompt-side encoders on libsvi_hip: they run once per clip and feed the DiT's `context` / `clip_feature`.

    WanTextEncoder     <- diffsynth/models/wan_video_text_encoder.py:209-256 (umT5-XXL encoder), called by
                          WanPrompter.encode_prompt (prompters/wan_prompter.py:99-112) as `self.text_encoder(ids, mask)`
    WanImageEncoder    <- diffsynth/models/wan_video_image_encoder.py:852-880, `encode_image(videos)`, called by
                          encode_images_adaptive (pipelines/svi_video.py:317) with the module switched to fp32 (:307-309)

The tokenizer (HuggingfaceTokenizer over the umt5-xxl sentencepiece files) stays the reference's: token ids are this boundary's input.
Dropout is the identity (the pipelines run the encoders in eval mode).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, List, Optional

import torch

from . import _lib as L


def relative_position_buckets(num_buckets: int, max_dist: int, length: int) -> List[int]:
    """T5RelativeEmbedding._relative_position_bucket (text_encoder:175-194, bidirectional) for rel = key - query in
    -(length-1) .. length-1, as the C side tabulates it (host only: no GPU needed)."""
    out = (C.c_int32 * (2 * length - 1))()
    L.check(L.lib().svi_t5_relative_buckets(num_buckets, max_dist, length, out), "svi_t5_relative_buckets")
    return list(out)


class _Encoder:
    """The handle of one native encoder: svi_<_ABI>_create / _bind_weight / _check_bound / _destroy, parameters of one dtype kept alive here."""
    _ABI, _NOUN, _DTYPE, _CODE = "", "", torch.float32, L.SVI_F32

    def _create(self, cfg) -> None:
        h = C.c_void_p()
        L.check(getattr(L.lib(), f"svi_{self._ABI}_create")(C.byref(cfg), C.byref(h)), f"svi_{self._ABI}_create")
        self._h = h
        self._params: Dict[str, torch.Tensor] = {}

    def bind(self, state_dict: Dict[str, torch.Tensor]) -> None:
        fn = getattr(L.lib(), f"svi_{self._ABI}_bind_weight")
        for name, t in state_dict.items():
            if not t.is_cuda or t.dtype != self._DTYPE or not t.is_contiguous():
                raise RuntimeError(f"{self._NOUN} parameter {name} must be a contiguous CUDA {self._DTYPE} tensor")
            shape = (C.c_int64 * t.dim())(*t.shape)
            L.check(fn(self._h, name.encode(), t.data_ptr(), self._CODE, shape, t.dim()), f"bind {name}")
            self._params[name] = t
        L.check(getattr(L.lib(), f"svi_{self._ABI}_check_bound")(self._h), f"svi_{self._ABI}_check_bound")

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                getattr(L.lib(), f"svi_{self._ABI}_destroy")(self._h)
                self._h = None
        except Exception:
            pass


class WanTextEncoder(_Encoder):
    """Mirror of the reference class of the same name; parameters are bf16 and borrowed."""
    _ABI, _NOUN, _DTYPE, _CODE = "t5", "text encoder", torch.bfloat16, L.SVI_BF16

    def __init__(self, vocab=256384, dim=4096, dim_attn=4096, dim_ffn=10240, num_heads=64, num_layers=24, num_buckets=32, shared_pos=False,
                 max_dist=128):
        self.vocab, self.dim, self.dim_attn, self.dim_ffn = vocab, dim, dim_attn, dim_ffn
        self.num_heads, self.num_layers, self.num_buckets, self.shared_pos = num_heads, num_layers, num_buckets, shared_pos
        self._create(L.T5Config(vocab, dim, dim_attn, dim_ffn, num_heads, num_layers, num_buckets, max_dist, int(bool(shared_pos))))

    @classmethod
    def from_state_dict(cls, state_dict: Dict[str, torch.Tensor], device="cuda", **overrides) -> "WanTextEncoder":
        sd = state_dict
        layers = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
        shared = "pos_embedding.embedding.weight" in sd
        pe = sd["pos_embedding.embedding.weight" if shared else "blocks.0.pos_embedding.embedding.weight"]
        cfg = dict(vocab=sd["token_embedding.weight"].shape[0], dim=sd["token_embedding.weight"].shape[1],
                   dim_attn=sd["blocks.0.attn.q.weight"].shape[0], dim_ffn=sd["blocks.0.ffn.fc1.weight"].shape[0],
                   num_heads=pe.shape[1], num_layers=layers, num_buckets=pe.shape[0], shared_pos=shared)
        cfg.update(overrides)
        m = cls(**cfg)
        m.bind({k: v.to(device=device, dtype=torch.bfloat16).contiguous() for k, v in sd.items()})
        return m

    @classmethod
    def from_module(cls, module) -> "WanTextEncoder":
        """An existing reference WanTextEncoder on the GPU in bf16: parameters are borrowed in place."""
        return cls.from_state_dict(dict(module.state_dict()))

    def forward(self, ids: torch.Tensor, mask: Optional[torch.Tensor] = None, rows: str = "all") -> torch.Tensor:
        """ids [B, L] integer, mask [B, L] (tokenizer padding: a prefix of ones) -> [B, L, dim] bf16.
        rows="all": every row as text_encoder(ids, mask) returns it; rows="valid": only the unpadded rows are computed, the rest is zero —
        exactly what encode_prompt keeps (prompter:110-111) at a fraction of the work."""
        if ids.dim() != 2:
            raise ValueError(f"ids must be [B, L] (got {tuple(ids.shape)})")
        B, Ln = ids.shape
        ids = ids.to(device="cuda", dtype=torch.int64).contiguous()
        if bool(((ids < 0) | (ids >= self.vocab)).any()):
            raise IndexError("token id out of range of the embedding table")
        if mask is None:
            valid = [Ln] * B
        else:
            if tuple(mask.shape) != (B, Ln):
                raise ValueError(f"mask must be [B, L] = {(B, Ln)} (got {tuple(mask.shape)})")
            mk = mask.to("cpu").gt(0)
            valid = [int(v) for v in mk.sum(dim=1)]
            for b, v in enumerate(valid):
                if v < 1 or not bool(mk[b, :v].all()):
                    raise ValueError("mask must be a non-empty prefix mask (tokenizer padding on the right)")
        out = torch.empty((B, Ln, self.dim), dtype=torch.bfloat16, device=ids.device)
        for b in range(B):
            r = Ln if rows == "all" else valid[b]
            L.check(L.lib().svi_t5_forward(self._h, L.ptr(ids[b]), Ln, valid[b], r, L.ptr(out[b]), L.current_stream()), "svi_t5_forward")
        return out

    __call__ = forward


class WanImageEncoder(_Encoder):
    """Mirror of the reference class of the same name (the visual tower of open-clip XLM-R ViT-H/14, all but the last block)."""
    _ABI, _NOUN = "clip", "image encoder"

    def __init__(self, image_size=224, patch_size=14, dim=1280, mlp_ratio=4, num_heads=16, num_layers=32, layers_used=None, norm_eps=1e-5):
        self.image_size, self.patch_size, self.dim, self.num_heads, self.num_layers = image_size, patch_size, dim, num_heads, num_layers
        used = num_layers - 1 if layers_used is None else layers_used                      # use_31_block=True (image_encoder:877)
        self._create(L.ClipConfig(image_size, patch_size, dim, mlp_ratio, num_heads, num_layers, used, norm_eps))
        self.tokens = (image_size // patch_size) ** 2 + 1

    @classmethod
    def from_state_dict(cls, state_dict: Dict[str, torch.Tensor], device="cuda", **cfg) -> "WanImageEncoder":
        """Keys of WanImageEncoder ("model.visual.…"), of the open-clip checkpoint ("visual.…", image_encoder:894-902) or of the bare
        VisionTransformer; anything outside the visual tower is ignored.  Parameters are converted to fp32 copies owned here — the
        reference casts the module to fp32 for the call and back afterwards (svi_video.py:307-309, :361-362)."""
        sd = {}
        for k, v in state_dict.items():
            if k.startswith("model.visual."):
                k = k[len("model.visual."):]
            elif k.startswith("visual."):
                k = k[len("visual."):]
            elif k.startswith(("model.", "textual.", "log_scale")):
                continue
            sd[k] = v
        pw = sd["patch_embedding.weight"]
        layers = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("transformer."))
        auto = dict(patch_size=pw.shape[-1], dim=pw.shape[0], num_layers=layers,
                    mlp_ratio=sd["transformer.0.mlp.0.weight"].shape[0] // pw.shape[0],
                    image_size=int(round((sd["pos_embedding"].shape[1] - 1) ** 0.5)) * pw.shape[-1])
        auto.update(cfg)
        m = cls(**auto)
        m.bind({k: v.to(device=device, dtype=torch.float32).contiguous() for k, v in sd.items()})
        return m

    @classmethod
    def from_module(cls, module, **cfg) -> "WanImageEncoder":
        vis = module.model.visual
        return cls.from_state_dict(dict(vis.state_dict()), num_heads=vis.num_heads, norm_eps=vis.norm_eps, **cfg)

    def encode_image(self, videos: Iterable[torch.Tensor]) -> torch.Tensor:
        """videos: list of [b, 3, H, W] tensors in [-1, 1] -> fp32 [sum b, tokens, dim] (hidden states after the last-but-one block)."""
        outs = []
        for u in videos:
            if u.dim() != 4 or u.shape[1] != 3:
                raise ValueError(f"each image batch must be [b, 3, H, W] (got {tuple(u.shape)})")
            x = u.to(device="cuda", dtype=torch.float32).contiguous()
            b, _, H, W = x.shape
            out = torch.empty((b, self.tokens, self.dim), dtype=torch.float32, device=x.device)
            L.check(L.lib().svi_clip_encode_image(self._h, L.ptr(x), b, H, W, L.ptr(out), L.current_stream()), "svi_clip_encode_image")
            outs.append(out)
        return torch.cat(outs) if len(outs) != 1 else outs[0]


W2V_CONV_KERNEL, W2V_CONV_STRIDE = (10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2)
W2V_STAGES = dict(wave=0, interp=8, proj=9, pos=10, enc_ln=11)          # conv layer i: 1 + i; block l: 12 + l (svi_w2v_forward_stage)
_W2V_POS = "encoder.pos_conv_embed.conv."
W2V_DEFAULT_MAX_FRAMES = 2048            # a fresh handle's frame limit: the resident encoder attention's key count, about 81 s of audio
W2V_FRAME_CAP = 65536                    # W2V_FRAME_CAP of csrc/svi_wav2vec.hip (= SVI_ENC_MAX_KEYS, csrc/svi_common.h): the most max_frames can be (43.7 min at 25 frames per second)


def audio_frames(n_samples: int) -> int:
    """Frames the wav2vec2 convolution stack makes of n_samples samples (host only: no GPU needed); 0 below its 400-sample receptive field."""
    out = C.c_int64(0)
    L.check(L.lib().svi_w2v_frames(int(n_samples), C.byref(out)), "svi_w2v_frames")
    return out.value


def fold_weight_norm(state_dict: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The positional convolution's weight norm (nn.utils.weight_norm(conv, name="weight", dim=2)) folded into a plain
    "encoder.pos_conv_embed.conv.weight" = v * g / ||v|| with the norm over all dimensions but the kernel's, in fp32.  Both spellings are read:
    weight_g / weight_v (torch.nn.utils.weight_norm) and parametrizations.weight.original0 / original1 (the parametrization API).  A state dict
    that already holds the plain weight is returned as it is.  Folded on the host whatever device the pair arrives on: one checkpoint gives the same
    bits whether it was read to the CPU or straight into HBM."""
    sd = dict(state_dict)
    for g_key, v_key in ((_W2V_POS + "weight_g", _W2V_POS + "weight_v"),
                         (_W2V_POS + "parametrizations.weight.original0", _W2V_POS + "parametrizations.weight.original1")):
        if g_key in sd or v_key in sd:
            if g_key not in sd or v_key not in sd:
                raise KeyError(f"audio encoder: {g_key} and {v_key} come as a pair")
            g, v = sd.pop(g_key).float().cpu(), sd.pop(v_key).float().cpu()
            if g.dim() != 3 or g.shape[0] != 1 or g.shape[1] != 1 or g.shape[2] != v.shape[2]:
                raise ValueError(f"audio encoder: weight norm over dim 2 expected, g is {tuple(g.shape)} for v {tuple(v.shape)}")
            sd[_W2V_POS + "weight"] = v * (g / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt())
    return sd


class WanAudioEncoder(_Encoder):
    """The talk variant's audio encoder on the device: wav2vec2-base as utils/audio_process.py:18-41 get_embedding runs it
    (utils/src/audio_analysis/wav2vec2.py Wav2Vec2Model.forward with seq_len and output_hidden_states=True), fp32; parameters are fp32 copies
    owned here.  The input is the ALREADY loudness-normalised 16 kHz mono array: loudness normalisation (pyloudnorm) and reading wav / mp4 files
    stay with the caller.

    max_frames: the most frames one encode() serves.  None keeps the handle's 2048 (about 81 s at 25 frames per second: the resident attention kernel);
    up to W2V_FRAME_CAP for longer audio — the reference encodes a file in one call, so a long file cannot be encoded in pieces.  Results of at most
    2048 frames do not depend on it, bit for bit."""

    FRAME_CAP = W2V_FRAME_CAP
    _ABI, _NOUN = "w2v", "audio encoder"

    def __init__(self, conv_dim=512, hidden=768, ffn=3072, num_heads=12, num_layers=12, pos_kernel=128, pos_groups=16, eps=1e-5, max_frames=None):
        self.conv_dim, self.hidden, self.ffn, self.num_heads, self.num_layers = conv_dim, hidden, ffn, num_heads, num_layers
        self.pos_kernel, self.pos_groups, self.eps = pos_kernel, pos_groups, eps
        self._create(L.W2vConfig(conv_dim, hidden, ffn, num_heads, num_layers, pos_kernel, pos_groups, eps))
        self._max_frames = W2V_DEFAULT_MAX_FRAMES
        if max_frames is not None:
            self.max_frames = max_frames

    @property
    def max_frames(self) -> int:
        """The most frames (seq_len) one encode() or stage() call serves."""
        return self._max_frames

    @max_frames.setter
    def max_frames(self, value: int) -> None:
        L.check(L.lib().svi_w2v_set_max_frames(self._h, int(value)), "svi_w2v_set_max_frames")
        self._max_frames = int(value)

    @staticmethod
    def config_from(config) -> dict:
        """Constructor arguments from a Wav2Vec2Config, or the dict of its config.json; only the architecture this backend runs is accepted."""
        get = (lambda k, d=None: config.get(k, d)) if isinstance(config, dict) else (lambda k, d=None: getattr(config, k, d))
        dims = list(get("conv_dim", (512,) * 7))
        if tuple(get("conv_kernel", W2V_CONV_KERNEL)) != W2V_CONV_KERNEL or tuple(get("conv_stride", W2V_CONV_STRIDE)) != W2V_CONV_STRIDE or \
                len(set(dims)) != 1 or len(dims) != 7:
            raise ValueError("audio encoder: the convolution stack must be seven layers of one width with kernels (10,3,3,3,3,2,2) and strides (5,2,2,2,2,2,2)")
        if get("feat_extract_norm", "group") != "group" or get("conv_bias", False) or get("do_stable_layer_norm", False) or get("add_adapter", False):
            raise ValueError("audio encoder: only the base layout is supported (group norm after the first convolution, bias-free convolutions, post-norm blocks, no adapter)")
        if get("hidden_act", "gelu") != "gelu" or get("feat_extract_activation", "gelu") != "gelu":
            raise ValueError("audio encoder: only the exact GELU activation is supported")
        return dict(conv_dim=dims[0], hidden=get("hidden_size", 768), ffn=get("intermediate_size", 3072), num_heads=get("num_attention_heads", 12),
                    num_layers=get("num_hidden_layers", 12), pos_kernel=get("num_conv_pos_embeddings", 128),
                    pos_groups=get("num_conv_pos_embedding_groups", 16), eps=get("layer_norm_eps", 1e-5))

    @classmethod
    def from_state_dict(cls, state_dict: Dict[str, torch.Tensor], config, device="cuda", max_frames=None) -> "WanAudioEncoder":
        """state_dict: Wav2Vec2Model's keys (a "wav2vec2." prefix of a task head's checkpoint is stripped, its other keys are skipped); config: a
        Wav2Vec2Config or the dict of config.json.  The positional convolution's weight norm is folded here (fold_weight_norm)."""
        sd = {}
        for k, v in state_dict.items():
            if k.startswith("wav2vec2."):
                k = k[len("wav2vec2."):]
            if k.startswith(("feature_extractor.", "feature_projection.", "encoder.")):
                sd[k] = v
        m = cls(**cls.config_from(config), max_frames=max_frames)
        m.bind({k: v.to(device=device, dtype=torch.float32).contiguous() for k, v in fold_weight_norm(sd).items()})
        return m

    @classmethod
    def from_module(cls, hf_model, device="cuda", max_frames=None) -> "WanAudioEncoder":
        """An existing (reference) Wav2Vec2Model: its parameters are copied to fp32 tensors on the device."""
        return cls.from_state_dict(dict(hf_model.state_dict()), hf_model.config, device=device, max_frames=max_frames)

    @staticmethod
    def _samples(speech) -> torch.Tensor:
        x = torch.as_tensor(speech)
        if x.dim() != 1:
            raise ValueError(f"speech must be a 1-D array of samples (got {tuple(x.shape)})")
        return x.to(device="cuda", dtype=torch.float32).contiguous()

    @staticmethod
    def seq_len(n_samples: int, sr: int = 16000) -> int:
        """int(audio_duration * 25) of get_embedding (audio_process.py:19-20, :31), in its double arithmetic."""
        return int(n_samples / sr * 25)

    def encode(self, speech, sr: int = 16000, dtype: torch.dtype = torch.float32, seq_len: Optional[int] = None) -> torch.Tensor:
        """speech: 1-D float tensor or ndarray, the loudness-normalised 16 kHz mono audio -> [N, num_layers, hidden] on the GPU (N = int(seconds * 25),
        or seq_len: the reference class's own argument), fp32 or bf16: the `audio_emb` of TalkStreamLoop.run and WanDiT.stage_audio_windows."""
        if sr != 16000:
            raise ValueError(f"the audio encoder reads 16 kHz audio (got sr = {sr}); resample first")
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"dtype must be torch.float32 or torch.bfloat16 (got {dtype})")
        x = self._samples(speech)
        n = x.numel()
        S = self.seq_len(n, sr) if seq_len is None else int(seq_len)
        out = torch.empty((max(S, 0), self.num_layers, self.hidden), dtype=dtype, device=x.device)
        L.check(L.lib().svi_w2v_forward(self._h, L.ptr(x) or 16, n, S, L.ptr(out) or 16, L.SVI_F32 if dtype == torch.float32 else L.SVI_BF16,
                                        L.current_stream()), "svi_w2v_forward")
        return out

    __call__ = encode

    def stage(self, speech, stage, seq_len: Optional[int] = None) -> torch.Tensor:
        """One intermediate tensor of encode(speech), fp32 (tests and inspection): stage = a W2V_STAGES name, ("conv", i) or ("layer", l)."""
        x = self._samples(speech)
        n = x.numel()
        S = self.seq_len(n) if seq_len is None else int(seq_len)
        if isinstance(stage, tuple):
            kind, i = stage
            code = {"conv": 1, "layer": 12}[kind] + int(i)
            if kind == "conv":
                frames = n
                for k, s in list(zip(W2V_CONV_KERNEL, W2V_CONV_STRIDE))[:i + 1]:
                    frames = (frames - k) // s + 1
                shape = (frames, self.conv_dim)
            else:
                shape = (S, self.hidden)
        else:
            code = W2V_STAGES[stage]
            shape = {"wave": (n,), "interp": (S, self.conv_dim)}.get(stage, (S, self.hidden))
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
        L.check(L.lib().svi_w2v_forward_stage(self._h, L.ptr(x), n, S, code, L.ptr(out), out.numel(), L.current_stream()), "svi_w2v_forward_stage")
        return out
