"""Operator seams of the reference, served by the HIP kernels.

Same names and argument meaning as the reference's own functions so that parity tests read like
calls into the reference:
    flash_attention(q, k, v, num_heads)                    models/wan_video_dit.py:116-147
    modulate / LayerNorm  -> layernorm_modulate            models/wan_video_dit.py:150-151,331-333
    RMSNorm + rope_apply  -> rmsnorm_rope                  models/wan_video_dit.py:186-197,178-183
    nn.Linear (+ fused epilogues) -> linear                models/wan_video_dit.py:227-229,242,334-335
    CFG combine + FlowMatchScheduler.step -> cfg_step      pipelines/svi_video.py:410,420
All tensors must be CUDA(HIP) bf16 and contiguous unless noted.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib as L


def _chk(t: torch.Tensor, name: str, dtype=torch.bfloat16):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (svi_hip has no CPU path)")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


def flash_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, num_heads: int,
                    compatibility_mode: bool = False) -> torch.Tensor:
    """[b, s, (n d)] layout in and out; d = 128."""
    _chk(q, "q"); _chk(k, "k"); _chk(v, "v")
    b, sq, dim = q.shape
    skv = k.shape[1]
    out = torch.empty_like(q)
    L.check(L.lib().svi_attention_fwd(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(out), b, sq, skv, num_heads,
                                      dim // num_heads, L.current_stream()), "flash_attention")
    return out


def fp8_attention(enable: bool = True) -> None:
    """Opt-in, process-wide, NOT the reference's arithmetic: every long-sequence attention call (flash_attention above, the DiT's self-attention) quantises
    Q and K to MX e4m3 and takes QK^T on the scaled fp8 matrix path; softmax and P·V stay as they are.  The reference's own dispatch offers this place to a
    quantised-QK^T backend (models/wan_video_dit.py:116-147, SageAttention).  Same as SVI_ATTN_QK8=1 in the environment; loops that hold a captured step graph
    re-capture.  Separately toleranced: tests/test_gpu_attn_qk8.py."""
    L.set_switch("SVI_ATTN_QK8", 1 if enable else None)


def fp8_attention_enabled() -> bool:
    """What the LIBRARY parsed (svi_switch_state), not the environment of the moment: an environment edit without a reload changes nothing the kernels do."""
    return L.lib().svi_switch_state(b"SVI_ATTN_QK8") == 1


def layernorm_modulate(x: torch.Tensor, eps: float = 1e-6, weight: Optional[torch.Tensor] = None,
                       bias: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None,
                       scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """LayerNorm over the last dim [+ affine] [+ x*(1+scale)+shift]; shift/scale are [dim] vectors."""
    _chk(x, "x")
    dim = x.shape[-1]
    rows = x.numel() // dim
    out = torch.empty_like(x)
    for t, n in ((weight, "weight"), (bias, "bias"), (shift, "shift"), (scale, "scale")):
        if t is not None:
            _chk(t, n)
            if t.numel() != dim:
                raise ValueError(f"{n} must have {dim} elements")
    L.check(L.lib().svi_layernorm_modulate(L.ptr(x), L.ptr(out), rows, dim, eps, L.ptr(weight), L.ptr(bias),
                                           L.ptr(shift), L.ptr(scale), L.current_stream()), "layernorm_modulate")
    return out


def rmsnorm_rope_(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6, grid=None, num_heads: int = 0) -> torch.Tensor:
    """In place on x [rows, dim]: RMSNorm over dim, then 3-D RoPE for the (f, h, w) token grid if given."""
    _chk(x, "x"); _chk(weight, "weight")
    rows, dim = x.shape[-2], x.shape[-1]
    f, h, w = grid if grid is not None else (0, 0, 0)
    L.check(L.lib().svi_rmsnorm_rope(L.ptr(x), dim, rows, dim, L.ptr(weight), eps, 1 if grid is not None else 0,
                                      num_heads, f, h, w, L.current_stream()), "rmsnorm_rope")
    return x


def rmsnorm_rope_qk_(x: torch.Tensor, rows: int, dim: int, weight_q: torch.Tensor, weight_k: Optional[torch.Tensor] = None, eps: float = 1e-6,
                     out_scale_q: float = 1.0, out_scale_k: float = 1.0, rope: int = 0, grid=(0, 0, 0), row0: int = 0, period: int = 0,
                     ld: Optional[int] = None) -> int:
    """The DiT's q | k launch (svi_rmsnorm_rope_qk, include/svi_hip.h), in place on the first `rows` rows of x [>= rows, ld]: RMSNorm (+ RoPE) of the
    operand at columns [0, dim) and, with weight_k, of the one at [dim, 2 dim).  Returns the library's status as it is — 0, or what the launcher
    refused (svi_hip._lib.last_error() has the text); nothing is checked here beyond what keeps the call inside x."""
    _chk(x, "x"); _chk(weight_q, "weight_q")
    if weight_k is not None:
        _chk(weight_k, "weight_k")
    ld = x.shape[-1] if ld is None else ld
    if x.dim() != 2 or ld != x.shape[-1] or not 0 <= rows <= x.shape[0]:
        raise ValueError(f"x {tuple(x.shape)} does not hold {rows} rows of ld {ld}")
    f, h, w = grid
    return L.lib().svi_rmsnorm_rope_qk(L.ptr(x), ld, rows, dim, L.ptr(weight_q), L.ptr(weight_k), eps, out_scale_q, out_scale_k, rope, f, h, w,
                                       row0, period, L.current_stream())


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, epilogue: int = L.EPI_BIAS,
           gate: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
           transpose_out: bool = False) -> torch.Tensor:
    """y = epilogue(x @ weight.T + bias).  x [M, K], weight [N, K].  transpose_out returns y^T [N, M8]
    (M8 = M rounded up to 8; the form the attention kernel wants V in)."""
    _chk(x, "x"); _chk(weight, "weight")
    M, K = x.shape
    N = weight.shape[0]
    if bias is not None:
        _chk(bias, "bias")
    if gate is not None:
        _chk(gate, "gate", torch.float32)
    st = L.current_stream()
    if transpose_out:
        ld = (M + 7) // 8 * 8
        out = torch.zeros((N, ld), dtype=torch.bfloat16, device=x.device)
        L.check(L.lib().svi_gemm_bf16(L.ptr(weight), K, L.ptr(x), K, L.ptr(out), ld, N, M, K, L.ptr(bias), 1,
                                      epilogue, None, None, 0, st), "linear^T")
        return out
    ldc = (N + 7) // 8 * 8
    out = torch.empty((M, ldc), dtype=torch.bfloat16, device=x.device)
    if residual is not None:
        _chk(residual, "residual")
    L.check(L.lib().svi_gemm_bf16(L.ptr(x), K, L.ptr(weight), K, L.ptr(out), ldc, M, N, K, L.ptr(bias), 0, epilogue,
                                  L.ptr(gate), L.ptr(residual), residual.shape[-1] if residual is not None else 0, st),
            "linear")
    return out if ldc == N else out[:, :N].contiguous()


def cfg_step_(latents: torch.Tensor, cond: torch.Tensor, uncond: Optional[torch.Tensor], cfg_scale: float,
              dsigma: float) -> torch.Tensor:
    """latents += (uncond + cfg_scale*(cond-uncond)) * dsigma, in place, bf16 op-by-op rounding."""
    _chk(latents, "latents"); _chk(cond, "cond")
    if uncond is not None:
        _chk(uncond, "uncond")
    L.check(L.lib().svi_cfg_step(L.ptr(latents), L.ptr(cond), L.ptr(uncond), latents.numel(), float(cfg_scale),
                                 float(dsigma), L.current_stream()), "cfg_step")
    return latents


def fp8_e4m3_to_bf16(t: torch.Tensor) -> torch.Tensor:
    """bf16 copy of a float8_e4m3fn tensor (exact): the cast the reference's FP8 mode performs in front of every use
    (vram_management/layers.py:65-71), done once."""
    if t.dtype != torch.float8_e4m3fn:
        raise ValueError(f"expected a float8_e4m3fn tensor, got {t.dtype}")
    src = t.to(device="cuda").contiguous()
    out = torch.empty(src.shape, dtype=torch.bfloat16, device=src.device)
    L.check(L.lib().svi_fp8_e4m3_to_bf16(L.ptr(src.view(torch.uint8)), L.ptr(out), src.numel(), L.current_stream()), "fp8_e4m3_to_bf16")
    return out


def f32_to_fp8_e4m3(t: torch.Tensor) -> torch.Tensor:
    """float8_e4m3fn copy of an fp32 or bf16 tensor with the semantics of torch's own `t.to(torch.float8_e4m3fn)` (round to nearest even,
    subnormals to 2^-9, no saturation: above 464 -> NaN), on the device: what the reference's `load_models(torch_dtype=torch.float8_e4m3fn)`
    does to every parameter, and the cast a LoRA merge into fp8-stored weights ends in (svi_lora_merge_e4m3)."""
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"expected an fp32 or bf16 tensor, got {t.dtype}")
    src = t.to(device="cuda").contiguous()
    out = torch.empty(src.shape, dtype=torch.float8_e4m3fn, device=src.device)
    L.check(L.lib().svi_f32_to_fp8_e4m3(L.ptr(src), L.SVI_F32 if src.dtype == torch.float32 else L.SVI_BF16, L.ptr(out), src.numel(),
                                        L.current_stream()), "f32_to_fp8_e4m3")
    return out


def cfg3_step_(latents: torch.Tensor, cond: torch.Tensor, uncond: torch.Tensor, drop_text: torch.Tensor, text_scale: float, audio_scale: float,
               dsigma: float) -> torch.Tensor:
    """latents += (uncond + text_scale*(cond - drop_text) + audio_scale*(drop_text - uncond)) * dsigma, in place, bf16 op-by-op
    (the talk sampler's guidance, svi_video_talk.py:455-461)."""
    for t, n in ((latents, "latents"), (cond, "cond"), (uncond, "uncond"), (drop_text, "drop_text")):
        _chk(t, n)
    L.check(L.lib().svi_cfg3_step(L.ptr(latents), L.ptr(cond), L.ptr(uncond), L.ptr(drop_text), latents.numel(), float(text_scale),
                                  float(audio_scale), float(dsigma), L.current_stream()), "cfg3_step")
    return latents


def audio_windows(emb: torch.Tensor, start: int, T_latent: int):
    """The talk variant's clip audio windows, cut on the device (svi_audio_windows) = get_audio_embedding + preprocess_audio + .to(bfloat16)
    (svi_video_talk.py:412-446): emb fp32 or bf16 [N, ...] (one row per audio frame of the whole stream; [N, 12, 768] in the real model, the trailing
    sizes' product a multiple of 8), `start` = audio_start_idx, T_latent latent frames.  Returns bf16 (first [1, 5, ...], latter [T_latent - 1, 8, ...]):
    the row of video frame f, window position w is emb[clamp(start + f + w - 2, 0, N - 1)]."""
    if not emb.is_cuda:
        raise RuntimeError("emb must live on the GPU (svi_hip has no CPU path)")
    if emb.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"emb must be fp32 or bf16, got {emb.dtype}")
    if emb.dim() < 2 or not emb.is_contiguous():
        raise ValueError(f"emb must be a contiguous [N, ...] tensor (got {tuple(emb.shape)})")
    N, tail = emb.shape[0], tuple(emb.shape[1:])
    first = torch.empty((1, 5) + tail, dtype=torch.bfloat16, device=emb.device)
    latter = torch.empty((max(int(T_latent) - 1, 0), 8) + tail, dtype=torch.bfloat16, device=emb.device)
    L.check(L.lib().svi_audio_windows(L.ptr(emb), L.SVI_F32 if emb.dtype == torch.float32 else L.SVI_BF16, N, emb[0].numel(), int(start), int(T_latent),
                                      L.ptr(first), L.ptr(latter) if latter.numel() else None, L.current_stream()), "audio_windows")
    return first, latter


ENCODER_ATTENTION_KERNELS = {"auto": 0, "resident": 1, "streaming": 2}
ENCODER_ATTENTION_RESIDENT_KEYS = 2048      # the resident kernel's key count (whole score rows in LDS)
ENCODER_ATTENTION_KEY_TILE = 256            # ENC_KT of csrc/svi_encoder_kernels.hip: keys per tile of the streaming kernel
ENCODER_ATTENTION_MAX_KEYS = 65536          # W2V_FRAME_CAP of csrc/svi_wav2vec.hip: what svi_w2v_set_max_frames grants at most


def encoder_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: Optional[float] = None, kernel=0,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The audio encoder's attention as an operator (svi_encoder_attention_f32): O = softmax(scale q k^T) v per head, fp32 throughout.
    q [Lq, heads, D], k and v [Lk, heads, D], fp32 on the GPU, D in 32, 64, 80, 128; the last two dimensions contiguous, the row stride free (views
    into a [L, 3 heads D] q | k | v buffer are read in place).  scale=None: 1 / sqrt(D).  kernel 0 / "auto": what the audio encoder launches (resident up
    to 2048 keys, streaming above); 1 / "resident": whole score rows in LDS, at most 2048 keys; 2 / "streaming": key tiles of ENCODER_ATTENTION_KEY_TILE,
    running maximum and sum, any key count up to ENCODER_ATTENTION_MAX_KEYS.  out: an fp32 [Lq, heads, D] tensor or view of the same kind to write."""
    for t, n in ((q, "q"), (k, "k"), (v, "v")) + (((out, "out"),) if out is not None else ()):
        if not t.is_cuda:
            raise RuntimeError(f"{n} must live on the GPU (svi_hip has no CPU path)")
        if t.dtype != torch.float32:
            raise TypeError(f"{n} must be torch.float32, got {t.dtype}")
        if t.dim() != 3 or t.shape[0] < 1 or t.stride(2) != 1 or t.stride(1) != t.shape[2]:
            raise ValueError(f"{n} must be a non-empty [rows, heads, D] tensor whose last two dimensions are contiguous (got {tuple(t.shape)}, strides {t.stride()})")
    Lq, heads, D = q.shape
    if tuple(k.shape[1:]) != (heads, D) or tuple(v.shape) != tuple(k.shape):
        raise ValueError(f"k and v must be [Lk, {heads}, {D}] (got {tuple(k.shape)} and {tuple(v.shape)})")
    if out is None:
        out = torch.empty((Lq, heads, D), dtype=torch.float32, device=q.device)
    elif tuple(out.shape) != (Lq, heads, D):
        raise ValueError(f"out must be [{Lq}, {heads}, {D}] (got {tuple(out.shape)})")
    code = ENCODER_ATTENTION_KERNELS[kernel] if isinstance(kernel, str) else int(kernel)
    ld = lambda t: t.stride(0) if t.shape[0] > 1 else max(t.stride(0), heads * D)      # noqa: E731  (a single row has no stride to speak of)
    L.check(L.lib().svi_encoder_attention_f32(L.ptr(q), ld(q), L.ptr(k), ld(k), L.ptr(v), ld(v), L.ptr(out), ld(out), Lq, k.shape[0], heads, D,
                                              float(D) ** -0.5 if scale is None else float(scale), code, L.current_stream()), "encoder_attention")
    return out


def pose_window(pose_u8: torch.Tensor, k: int, num_frames: int, num_motion_frames: int, height: int, width: int,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The dance variant's clip pose window, cut on the device (svi_pose_window): pose_u8 uint8 [N, h, w, 3], the whole pose video as the video reader
    hands it over, -> fp32 [3, num_frames, height, width], values 0..255: the `humanpose_data` of clip k, as the reference's script builds it between two
    clips (test_svi_dance.py:215-227, 281-288: the last num_motion_frames poses carried over, the rest read on from a cursor that wraps; every frame
    resized with nearest-neighbour, padded to the centre).  The rule is stated in include/svi_hip.h.  Written into `out` when given."""
    if not pose_u8.is_cuda:
        raise RuntimeError("pose_u8 must live on the GPU (svi_hip has no CPU path)")
    if pose_u8.dtype != torch.uint8 or pose_u8.dim() != 4 or pose_u8.shape[0] < 1 or pose_u8.shape[3] != 3:
        raise ValueError(f"pose_u8 must be uint8 [N >= 1, h, w, 3] (got {pose_u8.dtype}, {tuple(pose_u8.shape)})")
    if not pose_u8.is_contiguous():
        raise ValueError("pose_u8 must be contiguous")
    N, h, w, _ = pose_u8.shape
    shape = (3, int(num_frames), int(height), int(width))
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=pose_u8.device)
    elif not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous CUDA fp32 tensor {shape} (got {out.dtype}, {tuple(out.shape)})")
    L.check(L.lib().svi_pose_window(L.ptr(pose_u8), L.ptr(out), N, h, w, shape[2], shape[3], shape[1], int(num_motion_frames), int(k),
                                    L.current_stream()), "pose_window")
    return out


def linear_row_stats(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, eps: float = 1e-6):
    """nn.Linear whose epilogue also leaves RMSNorm's statistic of the OUTPUT rows (svi_linear_row_stats): returns (y bf16 [M, N], rs fp32 [M] =
    rsqrt(mean(y^2) + eps), row_sumsq fp32 [N/64, M]).  The cross-attention query projection of the DiT block (dit:296) runs this way."""
    x, weight = _chk(x, "x"), _chk(weight, "weight")
    if bias is not None:
        bias = _chk(bias, "bias")
    M, K = x.shape
    N = weight.shape[0]
    y = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    ss = torch.empty((N // 64, M), dtype=torch.float32, device=x.device)
    rs = torch.empty((M,), dtype=torch.float32, device=x.device)
    L.check(L.lib().svi_linear_row_stats(L.ptr(x), K, L.ptr(weight), K, L.ptr(y), N, M, N, K, L.ptr(bias), float(eps), L.ptr(ss), M, L.ptr(rs),
                                         L.current_stream()), "linear_row_stats")
    return y, rs, ss


def frame_attention(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, num_heads: int, rows_per_frame: int, keys_per_frame: int = 32,
                    row0: int = 0) -> torch.Tensor:
    """The talk variant's per-frame attention (models/attention.py:318-371, a block-diagonal mask over frames) in one launch
    (svi_attention_frames_fwd): q bf16 [nrows, n*128] = rows [row0, row0 + nrows) of a sequence of frames of `rows_per_frame` rows; the rows of
    frame fr attend to keys [fr * keys_per_frame, (fr + 1) * keys_per_frame) of k bf16 [frames * keys_per_frame, n*128] and of vt bf16 [n*128, ldvt]
    (V transposed); scale head_dim^-0.5.  Returns [nrows, n*128]."""
    q, k, vt = _chk(q, "q"), _chk(k, "k"), _chk(vt, "vt")
    out = torch.empty((q.shape[0], num_heads * 128), dtype=torch.bfloat16, device=q.device)
    L.check(L.lib().svi_attention_frames_fwd(L.ptr(q), q.shape[1], L.ptr(k), k.shape[1], L.ptr(vt), vt.shape[1], L.ptr(out), out.shape[1], int(row0),
                                             q.shape[0], int(rows_per_frame), int(keys_per_frame), num_heads, L.current_stream()), "frame_attention")
    return out


def cross_attention(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, num_heads: int, s_kv: Optional[int] = None, q_rs: Optional[torch.Tensor] = None,
                    q_gain: Optional[torch.Tensor] = None, q_out_scale: float = 1.0, key_tail: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The DiT block's cross-attention over the prompt's (short) key axis (svi_cross_attention_fwd): q bf16 [Lq, n*128] — with q_rs / q_gain the RAW
    projection output, RMS-normalised and scaled as it is read; without them used as it is (it must carry softmax_scale*log2e) — k bf16 [Lk, n*128]
    normalised, vt bf16 [n*128, ldvt] = V transposed (columns >= Lk up to a multiple of 8 readable)."""
    q, k, vt = _chk(q, "q"), _chk(k, "k"), _chk(vt, "vt")
    Lq, Lk = q.shape[0], (s_kv if s_kv is not None else k.shape[0])
    out = torch.empty((Lq, num_heads * 128), dtype=torch.bfloat16, device=q.device)
    if q_rs is not None:
        q_rs, q_gain = _chk(q_rs, "q_rs", torch.float32), _chk(q_gain, "q_gain")
    if key_tail is not None:
        key_tail = _chk(key_tail, "key_tail", torch.int32)
    L.check(L.lib().svi_cross_attention_fwd(L.ptr(q), q.shape[1], L.ptr(k), k.shape[1], L.ptr(vt), vt.shape[1], L.ptr(out), out.shape[1], Lq, Lk, num_heads,
                                            L.ptr(key_tail), L.ptr(q_rs), L.ptr(q_gain), float(q_out_scale), L.current_stream()), "cross_attention")
    return out
