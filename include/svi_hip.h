/* svi_hip.h — C ABI of libsvi_hip.so: the MI355X (gfx950) native backend for the
 * Stable-Video-Infinity rolling-window denoising hot path (Wan DiT block stack + flow-match
 * step + Wan 3-D causal VAE).
 *
 * The reference (vita-epfl/Stable-Video-Infinity) has no FFI: its boundary is a Python call
 * surface.  Each entry point below names the reference function it stands in for
 * (paths relative to the reference's diffsynth/ package); INTEGRATION.md shows the ctypes stub
 * that binds it underneath the unchanged reference call surface.
 *
 * Conventions
 *   - Plain C: opaque handles, raw DEVICE pointers, sizes.  No torch / HIP types in signatures
 *     (svi_stream is a hipStream_t passed as void*; NULL = the null stream).
 *   - Ownership: the caller owns every tensor (weights, inputs, outputs).  The library borrows
 *     pointers for the duration of a call; weight pointers for the lifetime of the binding
 *     (re-bind after a LoRA merge or any .to()/offload that moves storage).  The library owns
 *     only its workspace (allocated at first use for a given problem size, never in steady state).
 *   - All work is enqueued on the caller's stream; no internal synchronisation in steady state.
 *   - Errors: integer status, never abort/throw across the ABI; message via svi_last_error()
 *     (thread-local).  There is NO CPU fallback: with no usable GPU every compute call fails.
 *   - Activations are bf16 (row-major, innermost dim contiguous) unless stated; accumulation fp32.
 *   - Handles are not thread-safe; one handle per device, driven from one host thread at a time.  What the library owns
 *     outside the handles — the attention kernels' per-workgroup flag words, the scratch of the operator-level seams
 *     (svi_attention_fwd, svi_layernorm_modulate, svi_rmsnorm_rope, svi_rmsnorm_rope_qk), the per-kernel LDS attributes, the event profiler's
 *     records — is keyed by (device, stream) and guarded by one mutex: two handles on two streams, or two host threads
 *     driving two streams, do not share a buffer (work on ONE stream is ordered, which is what protects a buffer between
 *     consecutive calls).  A stream that is being captured must have seen each call once before the capture (buffers are
 *     created on first use; creating one under capture is refused with a message).
 */
#ifndef SVI_HIP_H
#define SVI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVI_HIP_ABI_VERSION 13

typedef enum {
    SVI_OK = 0,
    SVI_ERR_INVALID = 1,      /* bad argument / shape */
    SVI_ERR_UNBOUND = 2,      /* a required weight was never bound */
    SVI_ERR_HIP = 3,          /* HIP runtime error (message has hipGetErrorString) */
    SVI_ERR_UNSUPPORTED = 4,  /* valid in the reference, not implemented here */
    SVI_ERR_OOM = 5
} svi_status;

typedef enum { SVI_BF16 = 0, SVI_F32 = 1, SVI_F16 = 2 /* LoRA operands only (svi_lora_merge_e4m3) */,
               SVI_E4M3 = 3 /* OCP e4m3fn bytes: the DiT blocks' Linear weights bound FP8-resident (svi_dit_bind_weight) */ } svi_dtype;

typedef void* svi_stream;
typedef struct svi_dit svi_dit;
typedef struct svi_vae svi_vae;

/* Constructor arguments of models/wan_video_dit.py:408-421 (WanModel.__init__). head_dim must be 128. */
typedef struct {
    int32_t dim, in_dim, ffn_dim, out_dim, text_dim, freq_dim;
    float eps;
    int32_t patch_t, patch_h, patch_w;
    int32_t num_heads, num_layers;
    int32_t has_image_input;
    int32_t enable_multitalk;   /* talk variant: per-block audio cross-attention + audio_proj (models/wan_video_dit.py:338-351,455-470) */
} svi_dit_config;

/* GEMM epilogues (fused; see svi_gemm_bf16). */
typedef enum {
    SVI_EPI_BIAS = 0,           /* C = bf16(acc + bias)                                   nn.Linear            */
    SVI_EPI_BIAS_GELU_TANH = 1, /* C = bf16(gelu_tanh(bf16(acc + bias)))                  ffn.0+GELU  dit:334  */
    SVI_EPI_BIAS_GATE_RES = 2,  /* C = bf16(res + bf16(gate[n] * bf16(acc + bias)))       dit:369,370,373      */
    SVI_EPI_BIAS_GELU_ERF = 3,  /* exact GELU                                             img_emb     dit:383  */
    SVI_EPI_BIAS_SILU = 4,      /* C = bf16(silu(bf16(acc+bias)))                         time_embedding       */
    SVI_EPI_BIAS_RELU = 5       /* C = bf16(relu(bf16(acc+bias)))                         AudioProjModel dit:97-106 */
} svi_epilogue;

const char* svi_last_error(void);
int32_t svi_abi_version(void);
/* Number of visible HIP devices (0 => every compute entry point will fail with SVI_ERR_HIP). */
int32_t svi_device_count(void);

/* A/B tooling: the library reads its environment switches (SVI_FLASH_KERNEL, SVI_FLASH_TWO_PASS, SVI_FLASH_M16, SVI_FLASH_SPLIT, SVI_GEMM_KERNEL, SVI_GEMM_GM, SVI_GEMM_PF, SVI_GEMM_W8_256,
 * SVI_CROSS_DEDUP, SVI_CROSS_FUSED, SVI_RMS_ROWS, SVI_QK_FUSED, SVI_MX8_FUSED, SVI_QK8_FUSED, SVI_VAE_EXACT_FP32, SVI_VAE_X2H, SVI_VAE_DMA, SVI_VAE_UP_PHASES, SVI_VAE_TILE_ORDER, SVI_VAE_PAIR, SVI_T5_BUCKETS — all of them select between kernels that
 * compute the same result, bit for bit or within the stated parity bounds — and SVI_WS_LIMIT_MB, a budget in MiB beyond which a DiT workspace is refused with
 * SVI_ERR_OOM as if the allocation had failed (callers that share the device; the stacked CFG pair then falls back to its unstacked form, same bits);
 * csrc/svi_common.h SviSwitches) once, at first use; tools that flip them inside one process
 * call this afterwards.  The product library has no switch that changes results — with ONE documented
 * exception, off by default: SVI_ATTN_QK8=1 selects the opt-in quantised-QK^T attention (every long-sequence attention call quantises Q and K to
 * MX e4m3, one E8M0 scale per 32 channels, and takes QK^T on v_mfma_scale_f32_32x32x64_f8f6f4; softmax and P·V unchanged).  Like svi_dit_ffn_mx8
 * below it is arithmetic the reference never performs — its attention dispatch (models/wan_video_dit.py:116-147) merely accepts a quantised-QK^T
 * backend as interchangeable — with its own oracle and stated tolerance (tests/test_gpu_attn_qk8.py) and its own bench line (bench.py --fp8-attn).
 * In that mode the DiT's RMSNorm + RoPE launch writes the e4m3 rows and block scales itself (SVI_QK8_FUSED=0: bf16 q | k + two quantiser launches; same bits). */
svi_status svi_switches_reload(void);
/* The value the library PARSED for a switch at its last (re)load — SVI_ATTN_QK8, SVI_CROSS_FUSED, SVI_CROSS_DEDUP, SVI_QK_FUSED, SVI_FLASH_TWO_PASS, SVI_FLASH_M16:
 * 1 / 0 — or -1 for any other name.  What the kernels do follows this, not the process environment of the moment. */
int32_t svi_switch_state(const char* name);

/* ------------------------------------------------------------------ DiT: whole model ------ */
/* WanModel(...) construction (weights are bound afterwards, by reference state-dict key). */
svi_status svi_dit_create(const svi_dit_config* cfg, svi_dit** out);
svi_status svi_dit_destroy(svi_dit* h);
/* name = reference state-dict key, e.g. "blocks.0.self_attn.q.weight" (models/wan_video_dit.py
 * module tree).  dtype must be SVI_BF16 (the pipelines run the DiT in bf16, pipelines/svi_video.py:259) — except the 2-D Linear weights inside
 * blocks.* (self_attn.{q,k,v,o}, cross_attn.{q,k,v,o,k_img,v_img}, ffn.{0,2}, audio_cross_attn.{q_linear,kv_linear,proj}), which may also be bound as
 * SVI_E4M3: the stored bytes of the reference's FP8 mode themselves, [out, in] contiguous.  Their GEMMs then widen the bytes to bf16 on the way into the
 * matrix pipe (svi_gemm_bf16_w8) — the same bits as binding the bf16 cast, one byte per parameter resident instead of two more.  A handle may mix both;
 * norms, biases, modulation, embedders and the head stay bf16.  shape is checked against the config. */
svi_status svi_dit_bind_weight(svi_dit* h, const char* name, const void* dev_ptr, svi_dtype dtype,
                               const int64_t* shape, int32_t rank);
/* Returns SVI_OK when every parameter the config requires has been bound; otherwise
 * SVI_ERR_UNBOUND with the first missing key in svi_last_error(). */
svi_status svi_dit_check_bound(svi_dit* h);

/* model_fn_wan_video(dit, x, timestep, context, clip_feature, y, add_condition)
 * (pipelines/svi_video.py:74-137; same math as WanModel.forward, models/wan_video_dit.py:486-567).
 *   x            bf16 [B, 16, T, H, W]           latents
 *   timestep     f32  [B]            (device)    flow-match timestep (pipelines/svi_video.py:397)
 *   context      bf16 [B, Lc, text_dim]          T5 embeddings (un-projected)
 *   clip_feature bf16 [B, 257, 1280] or NULL     I2V only
 *   y            bf16 [B, in_dim-16, T, H, W] or NULL   I2V only (mask ‖ VAE latent)
 *   add_condition bf16 [B, L, dim] or NULL       added to patch tokens (dance pose embedder)
 *   out          bf16 [B, out_dim, T, H, W]      velocity prediction
 * TeaCache and USP hooks of the reference function are not part of this entry point. */
svi_status svi_dit_forward(svi_dit* h, const void* x, const float* timestep, const void* context,
                           const void* clip_feature, const void* y, const void* add_condition,
                           void* out, int32_t B, int32_t T, int32_t H, int32_t W, int32_t Lc,
                           svi_stream stream);

/* Talk variant — model_fn_wan_talk_video (pipelines/svi_video_talk.py:83-160) = WanModel.forward with audio_embed_tuple
 * (models/wan_video_dit.py:486-567): the audio windows are projected to 32 context tokens of width 768 per latent frame
 * (AudioProjModel, dit:44-115) and every block adds, after its text cross-attention,
 *     x += proj(attention_per_frame(q_linear(norm_x(x)), kv_linear(audio tokens of the frame)))     (dit:361-366, models/attention.py:318-371)
 * svi_dit_set_audio arms the handle for the following forwards (svi_dit_forward / _forward_tea, and sequence shards: svi_dit_sp_begin projects
 * the audio tokens of ALL latent frames on every rank, and a shard's rows — which may start and end inside a frame — attend to their own frames'
 * tokens through svi_attention_frames_fwd's kernel, the single-rank bits; the CFG pair, svi_dit_forward_cfg_pair and svi_dit_sp_begin_pair, refuses
 * while audio is set: its branches differ in their audio — the three guidance forwards of a talk step are svi_dit_forward_talk3) and NULL pointers
 * disarm it:
 *   audio_first  bf16 [1, seq_len = 5, 12, 768]          the first frame's audio window          (audio_embed_tuple[0])
 *   audio_latter bf16 [T - 1, seq_len_vf = 8, 12, 768]   the later latent frames' windows        (audio_embed_tuple[1])
 * The pointers are borrowed until the next svi_dit_set_audio. */
svi_status svi_dit_set_audio(svi_dit* h, const void* audio_first, const void* audio_latter, int32_t n_latter);

/* The talk step as ONE call (additive in v13): the three guidance forwards of SVITalkVideoPipeline._sample_with_multitalk (svi_video_talk.py:455-458).
 *
 * svi_dit_audio_slot projects one clip's audio windows (shapes as svi_dit_set_audio) through AudioProjModel and through EVERY block's
 * audio_cross_attn.kv_linear into buffers the slot owns: AUD [f * 32, 768] and, per layer, K [f * 32, dim] and V^T [dim, ld] — the launches an armed
 * forward makes per forward and block, so the bits are a forward's.  They depend on (audio, weights) alone.  slot 0 = the clip's audio, 1 = the null
 * audio.  Stream-ordered; the caller's pointers are read by the work this call enqueues and are NOT borrowed.  The first staging of a slot, or one
 * with another frame count, allocates and moves svi_dit_generation (refused while the stream is being captured); a re-staging with the same frame count
 * rewrites the buffers in place — no address and no generation moves: the clip boundary of a resident loop, as svi_dit_context_refill is for the
 * prompt.  audio_first == NULL frees the slot (the generation moves).  Binding a weight drops both slots, as it drops the context cache.
 * Memory: per slot num_layers x 2 x (f * 32) x dim x 2 B — 40 x 2 x 672 x 5120 x 2 B = 0.55 GB at the 14B width with 21 latent frames, 1.1 GB for
 * the two slots a talk step needs.
 *
 * svi_dit_forward_talk3 runs, for one sample,
 *     out_cond      = forward(context_cond,   audio slot 0, add_condition)
 *     out_uncond    = forward(context_uncond, audio slot 1, no add_condition)
 *     out_drop_text = forward(context_uncond, audio slot 0, add_condition)
 * with the timestep embedding and modulation rows, patchify and the patch embedding computed once (the add_condition rows are added to a copy), block
 * 0's self-attention third once per distinct embedded input (one run when add_condition is NULL, else two: cond and drop-text share), and every
 * block's audio K / V^T read from the slots.  The branches then run one after another on the L-row workspace (three stacked branches would pass the
 * stacked form's 2 GiB bound at the talk model's size).  Each output is bit-identical to svi_dit_forward with that branch's audio armed.  Works with
 * the context cache on or off.  Once the slots are staged and a first call has sized the workspace (and, cache on, filled the prompts' entries) a call
 * allocates nothing and does not synchronise: it can be captured into a hipGraph.  Refused (SVI_ERR_INVALID, with a message): a model without
 * enable_multitalk; a slot that is not staged, or staged for another frame count than T / patch_t; audio armed through svi_dit_set_audio; NULL or
 * overlapping outputs; sizes not divisible by the patch. */
svi_status svi_dit_audio_slot(svi_dit* h, int32_t slot /* 0 or 1 */, const void* audio_first, const void* audio_latter, int32_t n_latter,
                              svi_stream stream);
svi_status svi_dit_forward_talk3(svi_dit* h, const void* x, const float* timestep, const void* context_cond, const void* context_uncond,
                                 const void* clip_feature, const void* y, const void* add_condition, void* out_cond, void* out_uncond,
                                 void* out_drop_text, int32_t T, int32_t H, int32_t W, int32_t Lc, svi_stream stream);
/* The clip boundary of a talk STREAM (additive in v13): the clip's audio windows cut on the device out of the whole stream's audio embedding.
 *
 * svi_audio_windows (the operator seam): emb [N, R] — one row per audio frame of the stream, fp32 (as the reference holds the wav2vec2 output) or bf16,
 * R = blocks x channels (12 x 768 in the real model; any R % 8 == 0) — is read for the clip that starts at audio frame `start` and has T_latent latent
 * frames (4 (T_latent - 1) + 1 video frames, window 5).  The row of (video frame f, window position w) is clamp(start + f + (w - 2), 0, N - 1):
 *   first_out  bf16 [1, 5, R]             video frame 0's five window rows                                            (audio_embed_tuple[0])
 *   latter_out bf16 [T_latent - 1, 8, R]  latent frame t = video frames 1 + 4t .. 4 + 4t: positions 0, 1, 2 of the first, the centre (2) of the two
 *                                         middle ones, positions 2, 3, 4 of the last; may be NULL when T_latent == 1 (audio_embed_tuple[1])
 * = SVITalkVideoPipeline.get_audio_embedding + preprocess_audio + .to(bfloat16) (pipelines/svi_video_talk.py:412-446): a clamped gather and one
 * round-to-nearest-even, so the result is defined bit for bit.  One launch, 16-byte accesses (operands 16-byte aligned).
 *
 * svi_dit_audio_slot_windows cuts the windows of the model's width (R = 12 x 768) into buffers slot `slot` owns and re-projects the slot from there
 * with svi_dit_audio_slot's launches — the bits of svi_dit_audio_slot on host-built windows.  Same rules as svi_dit_audio_slot: a slot that is staged
 * for T_latent frames is rewritten in place (nothing is allocated, svi_dit_generation does not move: legal between replays of a captured talk step);
 * otherwise it is (re)allocated (refused while the stream is being captured).  emb is read by the work this call enqueues and is not borrowed.
 *
 * Both refuse, with a message and before any launch: a NULL emb, N < 1, T_latent < 1, start < 0, a dtype other than fp32 / bf16; svi_audio_windows
 * also an R that is not a positive multiple of 8 or a NULL output. */
svi_status svi_audio_windows(const void* emb, svi_dtype dtype, int32_t N, int32_t R, int32_t start, int32_t T_latent, void* first_out,
                             void* latter_out, svi_stream stream);
svi_status svi_dit_audio_slot_windows(svi_dit* h, int32_t slot /* 0 or 1 */, const void* emb, svi_dtype dtype, int32_t N, int32_t start,
                                      int32_t T_latent, svi_stream stream);
/* The talk step with TeaCache (additive in v13): svi_dit_forward_talk3 plus svi_dit_forward_tea's modes, one per branch, and one residual bf16 [1, L, dim]
 * per branch.  Per branch k = cond, uncond, drop_text:
 *   0: run the blocks; residual_k is ignored (may be NULL).
 *   1 (store): run the blocks and write residual_k = bf16(x_after_blocks_k - x_before_blocks_k).
 *   2 (skip): run no block and read no audio slot; the head reads bf16(x_before_blocks_k + residual_k).
 * x_before_blocks_k is the branch's own embedded input: the patch embedding for uncond, bf16(patch embedding + add_condition) for cond and drop_text — two
 * branches that skip from the same residual still differ wherever add_condition is given.  Rounding points as svi_dit_forward_tea; all modes 0 is
 * svi_dit_forward_talk3 itself.
 * The reference consults ONE negative TeaCache object twice per step (svi_video_talk.py:448-466: uncond, then drop-text), so residual_uncond and
 * residual_drop_text may be THE SAME buffer.  The branches take effect in the order cond, uncond, drop_text on the caller's stream, and so do the reads and
 * writes of a shared buffer: a skipping drop_text reads what uncond stored in this call; a skipping uncond reads the old values before drop_text's store
 * overwrites them; of two stores drop_text's is what remains.
 * Shared among the branches that run their blocks, as in svi_dit_forward_talk3: the timestep stage and the patch embedding (once per call, also for the
 * skipping branches), block 0's self-attention once per distinct embedded input, the audio K / V^T of the slots.  The skipping branches are served by one
 * row kernel — a row of the patch embedding read once, the add_condition row where a skipping branch has one, each skipping branch's residual row; it writes
 * the head's LayerNorm + modulate row per branch with svi_dit_forward_tea's bits — then the head projection and unpatchify per branch.  uncond and drop_text
 * skipping from the same buffer without add_condition are equal by construction: computed once, written twice.
 * The patch embedding is kept in a buffer of its own, L x dim x 2 B (0.34 GB at 32760 tokens and the 14B width), allocated by the first call with a mode
 * other than 0 (svi_dit_generation moves; refused while the stream is being captured), so every mode pattern after it runs on the same addresses and can be
 * captured into a hipGraph.
 * Refused (SVI_ERR_INVALID, the message names the argument): a mode outside 0..2; a NULL or misaligned (16 B) residual where the mode is 1 or 2;
 * residual_cond overlapping either of the others; residual_uncond and residual_drop_text overlapping without being identical; a residual overlapping an
 * output, x or an audio slot; and everything svi_dit_forward_talk3 refuses — unstaged or mis-sized slots also when every branch skips, so that a mode
 * pattern cannot change which calls are legal.  Each output and residual is bit-identical to svi_dit_forward_tea calls in the order cond, uncond, drop_text
 * with that branch's audio armed. */
svi_status svi_dit_forward_talk3_tea(svi_dit* h, const void* x, const float* timestep, const void* context_cond, const void* context_uncond,
                                     const void* clip_feature, const void* y, const void* add_condition, void* out_cond, void* out_uncond,
                                     void* out_drop_text, int32_t T, int32_t H, int32_t W, int32_t Lc, int32_t tea_cond, int32_t tea_uncond,
                                     int32_t tea_drop_text, void* residual_cond, void* residual_uncond, void* residual_drop_text, svi_stream stream);

/* TeaCache support (pipelines/svi_video.py:23-72 class TeaCache, :117-131 its use inside model_fn_wan_video).
 * svi_dit_time_mod: t_mod bf16 [B, 6, dim], the tensor TeaCache.check() compares between steps (host logic decides).
 * svi_dit_forward_tea: svi_dit_forward with tea_mode 0 = plain; 1 = run the blocks and write
 *   residual bf16 [B, L, dim] = bf16(x_after_blocks - x_before_blocks)          (TeaCache.store, :64-66);
 *   2 = skip the blocks: x = bf16(x_patchified + residual), then the head       (TeaCache.update, :68-70). */
svi_status svi_dit_time_mod(svi_dit* h, const float* timestep, void* t_mod_out, int32_t B, svi_stream stream);
svi_status svi_dit_forward_tea(svi_dit* h, const void* x, const float* timestep, const void* context,
                               const void* clip_feature, const void* y, const void* add_condition, void* out,
                               int32_t B, int32_t T, int32_t H, int32_t W, int32_t Lc, int32_t tea_mode, void* residual,
                               svi_stream stream);

/* The two forwards of one classifier-free-guidance step — model_fn_wan_video(dit, latents, timestep, **prompt_emb_posi, ...) and
 * the same call with prompt_emb_nega (pipelines/svi_video.py:401-408) — in one call.  They share latents and timestep, so the
 * timestep embedding, patchify and block 0's self-attention (everything that precedes the first use of the prompt) are
 * computed once.  out_cond / out_uncond are bit-identical to two svi_dit_forward calls with the respective context. */
svi_status svi_dit_forward_cfg_pair(svi_dit* h, const void* x, const float* timestep, const void* context_cond,
                                    const void* context_uncond, const void* clip_feature, const void* y,
                                    const void* add_condition, void* out_cond, void* out_uncond, int32_t B, int32_t T,
                                    int32_t H, int32_t W, int32_t Lc, svi_stream stream);
/* The CFG pair with TeaCache: svi_dit_forward_cfg_pair plus svi_dit_forward_tea's modes, for both branches in one call (additive in v12).
 *   tea_mode 0: svi_dit_forward_cfg_pair, the residual arguments are ignored.
 *   tea_mode 1 (store): the pair forward, prefix shared as above, which also leaves residual_k bf16 [B, L, dim] = bf16(x_after_blocks_k - x_before_blocks)
 *     for k = cond, uncond.  x_before_blocks does not depend on the prompt: it is snapshotted once.
 *   tea_mode 2 (skip): timestep embedding and patch embedding once; one row kernel reads a row of x and the matching rows of both residuals, forms
 *     bf16(x + residual_k) — the rounding point of svi_dit_forward_tea's add — and writes the head's LayerNorm + modulate rows of both branches; the head
 *     projection runs once over the 2 L stacked rows (per branch where the stacked workspace is not in use), unpatchify per branch.  The contexts are not read.
 * Modes 1 and 2 need both residual buffers, distinct and 16-byte aligned; refusals otherwise as svi_dit_forward_cfg_pair (audio armed: SVI_ERR_UNSUPPORTED).
 * Per (sample, branch) the outputs and residuals are bit-identical to two svi_dit_forward_tea calls with the respective context and residual. */
svi_status svi_dit_forward_cfg_pair_tea(svi_dit* h, const void* x, const float* timestep, const void* context_cond,
                                        const void* context_uncond, const void* clip_feature, const void* y,
                                        const void* add_condition, void* out_cond, void* out_uncond, int32_t B, int32_t T,
                                        int32_t H, int32_t W, int32_t Lc, int32_t tea_mode, void* residual_cond, void* residual_uncond,
                                        svi_stream stream);

/* Hoists what depends only on the prompt out of the step loop (SURVEY §8 a2 / f N2): with the cache enabled
 * svi_dit_forward projects a context (text_embedding / img_emb, pipelines/svi_video.py:94-99) and computes every block's
 * cross-attention K / V^T (models/wan_video_dit.py:272-274) ONCE per distinct (context pointer, clip_feature pointer, Lc)
 * and reuses them; results are bit-identical to the uncached path.  The caller promises that the contents behind a cached
 * pointer do not change while the cache is on; svi_dit_context_cache(h, 0), or binding a weight, drops all entries
 * (4 entries, least recently used first). */
svi_status svi_dit_context_cache(svi_dit* h, int32_t enable);
/* The rolling window's clip boundary (test_svi.py:424-476: every clip re-enters SVIVideoPipeline.__call__ with the next prompt): the caller has
 * written the NEXT prompt's embedding (and CLIP feature) into the tensors a cache entry is keyed by; the entry is recomputed IN PLACE — projected
 * context, identical-suffix summary, every block's cross-attention K / V^T (models/wan_video_dit.py:272-274) — in the buffers it already owns.
 * No device address moves and svi_dit_generation does not, so a hipGraph of the step captured for the previous clip replays on the new prompt.
 * Stream-ordered.  Without an entry for (context, clip_feature, Lc) it is a first fill (allocates; the generation moves). */
svi_status svi_dit_context_refill(svi_dit* h, const void* context, const void* clip_feature, int32_t Lc, svi_stream stream);

/* Sequence-parallel (Ulysses) pieces of one forward — SURVEY §8e axis 3; the reference's USP path: the token chunk / all_gather of
 * pipelines/svi_video.py:119-135 and the all-to-all attention of distributed/xdit_context_parallel.py.  A rank owns token rows
 * [row0, row0 + nrows) of the (f h w) sequence for everything row-local and trades tokens for heads around self-attention; the
 * exchanges (RCCL all-to-all / all-gather) are the caller's, between these calls (svi_hip/sequence_parallel.py):
 *   svi_dit_sp_begin        timestep embedding, context (cache honoured), patchify of the rank's rows
 *   svi_dit_sp_block_qkv    block `layer`: LN + modulate, q | k projections, RMSNorm + RoPE at the rows' true positions (q pre-scaled by
 *                           softmax_scale*log2e) stored IN SEND ORDER: q_send / k_send bf16 [G][P][nrows][Dg] — destination rank j owns
 *                           channel block [j*Dp, (j+1)*Dp), Dp = dim/P, split into G head groups of Dg = Dp/G channels — so each
 *                           (operand, head group) is one contiguous all-to-all input; V^T -> vt_out bf16 [dim, ldvt] (cols >= nrows
 *                           untouched), whose row block j is rank j's piece.  No packing pass on either side of the exchange.
 *   svi_sp_unpack_vt        received V^T pieces [P(src)][Dp][lds] -> [Dp][L8] (token axis source-major)
 *   svi_sp_unpack_out       received attention pieces [G][P(src)][nrows][Dg] -> attn bf16 [nrows, dim]
 *   svi_attention_vt_fwd    attention of a head group on those layouts (after the exchange: all tokens, n = heads/P)
 *   svi_dit_sp_block_rest   attn bf16 [nrows, dim] (after the exchange back) -> output projection + gate + residual,
 *                           cross-attention, MLP of block `layer`
 *   svi_dit_sp_head         head rows bf16 [nrows, svi_dit_head_ld]; all-gathered, then svi_dit_unpatchify -> [out_dim, T, H, W]
 * With one rank (row0 = 0, nrows = L) the sequence is bit-identical to svi_dit_forward.  With audio armed (svi_dit_set_audio) the talk variant runs on
 * the shard: the windows must cover the whole sequence's T / patch_t latent frames, as on one rank. */
svi_status svi_dit_sp_begin(svi_dit* h, const void* x, const float* timestep, const void* context, const void* clip_feature,
                            const void* y, const void* add_condition, int32_t T, int32_t H, int32_t W, int32_t Lc,
                            int32_t row0, int32_t nrows, svi_stream stream);
/* Both forwards of a CFG step on one shard, STACKED (svi_dit_forward_cfg_pair's form on a rank's rows; needs svi_dit_context_cache(h, 1)): the shard's
 * rows of the conditional branch on top of the unconditional branch's.  The calls that follow act on 2 nrows rows: svi_dit_sp_block_qkv stores
 * q_send / k_send as [G][P][nrows][branch][Dg] and V^T as [dim, ldvt >= 2 nrows] (columns [0, nrows) conditional, [nrows, 2 nrows) unconditional);
 * svi_dit_sp_block_rest takes attn [2 nrows, dim]; svi_dit_sp_head writes [2 nrows, svi_dit_head_ld].  After the exchange the two branches are twice as
 * many heads of one svi_attention_vt_fwd call per head group (row stride 2 Dg).
 * No CFG exchange between ranks; each row-local launch of a shard is twice as long.  Bit-identical to two svi_dit_sp_begin forwards. */
svi_status svi_dit_sp_begin_pair(svi_dit* h, const void* x, const float* timestep, const void* context_cond, const void* context_uncond,
                                 const void* clip_feature, const void* y, const void* add_condition, int32_t T, int32_t H, int32_t W, int32_t Lc,
                                 int32_t row0, int32_t nrows, svi_stream stream);
/* svi_dit_sp_block_qkv_part: the same in two pieces — part 1 = LN + modulate and the V^T projection, part 2 = the q | k projection with RMSNorm + RoPE
 * (0 = both: svi_dit_sp_block_qkv) — so that V^T can be on the wire while q | k are still being made (the gather mode of sequence_parallel.py). */
svi_status svi_dit_sp_block_qkv_part(svi_dit* h, int32_t layer, void* q_send, void* k_send, void* vt_out, int32_t ldvt, int32_t P, int32_t G,
                                     int32_t part, svi_stream stream);
svi_status svi_dit_sp_block_qkv(svi_dit* h, int32_t layer, void* q_send, void* k_send, void* vt_out, int32_t ldvt, int32_t P, int32_t G,
                                svi_stream stream);
/* nb = CFG branches stacked on the shard (1, or 2 after svi_dit_sp_begin_pair): a token's branches travel side by side, so what a rank receives per head
 * group is token-major [L, nb * Dg] and the branches' heads are nb x as many heads of ONE attention launch.  svi_sp_unpack_vt: a piece's columns hold branch b's
 * tokens at [b * Ls, (b + 1) * Ls); channel g * Dg + cg goes to row (g * nb + b) * Dg + cg of out [G * nb * Dg][L8] (Dg = channels per head group; nb = 1:
 * row = channel).  svi_sp_unpack_out: pieces [G][P(src)][Ls][nb][Dg] -> attn [nb * Ls][dim], branch b's rows at [b * Ls, (b + 1) * Ls). */
svi_status svi_sp_unpack_vt(const void* recv, void* out, int32_t P, int32_t Dp, int32_t Ls, int32_t lds, int32_t L8, int32_t nb, int32_t Dg, svi_stream stream);
svi_status svi_sp_unpack_out(const void* recv, void* out, int32_t P, int32_t G, int32_t Ls, int32_t Dg, int32_t nb, svi_stream stream);
svi_status svi_dit_sp_block_rest(svi_dit* h, int32_t layer, const void* attn, svi_stream stream);
/* TeaCache on a shard's rows (the reference combines TeaCache and USP, pipelines/svi_video.py:112-131): mode 0 snapshot before the blocks,
 * 1 residual bf16 [nrows, dim] = x_after - x_before, 2 x += residual in place of the blocks. */
svi_status svi_dit_sp_tea(svi_dit* h, int32_t mode, void* residual, svi_stream stream);
svi_status svi_dit_sp_head(svi_dit* h, void* head_rows_out, svi_stream stream);
svi_status svi_dit_unpatchify(svi_dit* h, const void* head_rows, void* out, int32_t T, int32_t H, int32_t W, svi_stream stream);
int32_t svi_dit_head_ld(svi_dit* h);
/* Moves whenever device state that a captured hipGraph of this handle's forwards may have baked in stops being valid (workspace
 * growth, a context-cache entry filled or evicted, svi_dit_context_cache, a weight re-bound, a per-stream library buffer freed).  Read it
 * right after a capture; replay only while it is unchanged (svi_hip.DenoiseLoop does). */
int64_t svi_dit_generation(svi_dit* h);
/* The library keeps small device buffers per (device, stream) — the attention kernels' flag words, split-key partial sums — for as long as
 * the process lives.  A caller that retires a stream (a hipGraph capture stream) releases them here; all_streams != 0: those of every stream
 * of the current device.  Drains the device.  Graphs captured on the stream must not be replayed afterwards (svi_dit_generation moves). */
svi_status svi_stream_buffers_release(svi_stream stream, int32_t all_streams);
svi_status svi_attention_vt_fwd(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* vt, int32_t ldvt, void* out,
                                int32_t ldo, int32_t s_q, int32_t s_kv, int32_t n, int32_t q_prescaled, svi_stream stream);
/* Frame-segmented attention (the talk variant's audio cross-attention, models/attention.py:318-371: a block-diagonal mask over frames) in ONE launch:
 * q / out hold nrows rows, rows [row0, row0 + nrows) of a sequence of frames of rows_per_frame rows (q points at row row0); the rows of frame fr attend
 * to keys [fr * keys_per_frame, (fr + 1) * keys_per_frame) of k [frames * keys_per_frame, ldk] and of vt [n*128, ldvt] (V transposed; both point at
 * frame 0's keys; ldvt >= keys of every frame the range touches); scale head_dim^-0.5 on q as it is.  keys_per_frame % 8 == 0.  A range may start
 * and end inside a frame.  Per row the same bits as svi_attention_vt_fwd(q_prescaled = 0) launched once per frame segment of the range. */
svi_status svi_attention_frames_fwd(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* vt, int32_t ldvt, void* out, int32_t ldo,
                                    int32_t row0, int32_t nrows, int32_t rows_per_frame, int32_t keys_per_frame, int32_t n, svi_stream stream);

/* CrossAttention.forward's query path (models/wan_video_dit.py:296,299: q = norm_q(self.q(x)); x = attn(q, k, v)) as the DiT block runs it by default:
 *   svi_linear_row_stats    C = bf16(A W^T + bias) [M, N] AND the statistic of RMSNorm over the full width (dit:192-197): row_sumsq [N/64][ldss] = sums of
 *                           squares of the rounded results per aligned 64-column group (left by the GEMM's epilogue: fixed summation tree, the same in every
 *                           tile kernel), rs_out[m] = rsqrt(sum_g row_sumsq[g][m] / N + eps).
 *   svi_cross_attention_fwd softmax(q' k^T) v over a SHORT key axis (the prompt) with q' = bf16(bf16(bf16(q q_rs[row]) q_gain) q_out_scale) formed as the rows
 *                           are read (q_rs NULL: q is used as it is; either way q carries softmax_scale*log2e already); vt = V transposed [n*128, ldvt];
 *                           key_tail as in svi_dit's cross-attention (device {n, m}: keys n-1.. identical, counted m times) or NULL.  One [s_q, n*128] read and
 *                           one write per call — the separately normalised q never exists in memory. */
svi_status svi_linear_row_stats(const void* A, int32_t lda, const void* W, int32_t ldw, void* C, int32_t ldc, int32_t M, int32_t N, int32_t K,
                                const void* bias, float eps, float* row_sumsq, int32_t ldss, float* rs_out, svi_stream stream);
svi_status svi_cross_attention_fwd(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* vt, int32_t ldvt, void* out, int32_t ldo,
                                   int32_t s_q, int32_t s_kv, int32_t n, const int32_t* key_tail, const float* q_rs, const void* q_gain,
                                   float q_out_scale, svi_stream stream);

/* DiTBlock.forward(x, context, t_mod, freqs) for block `layer` (models/wan_video_dit.py:354-374).
 *   x_inout bf16 [L, dim] (L = f*h*w, updated in place); context bf16 [Lc(+257), dim] ALREADY
 *   projected by text_embedding/img_emb; t_mod bf16 [6, dim]; freqs implied by the (f,h,w) grid. */
svi_status svi_dit_block_forward(svi_dit* h, int32_t layer, void* x_inout, const void* context,
                                 const void* t_mod, int32_t f, int32_t hh, int32_t ww, int32_t Lc,
                                 svi_stream stream);

/* ------------------------------------------------------------------ operator seams -------- */
/* flash_attention(q, k, v, num_heads) (models/wan_video_dit.py:116-147): layout [b, s, (n d)],
 * unmasked softmax(q k^T / sqrt(d)) v, d must be 128.  out may not alias the inputs. */
svi_status svi_attention_fwd(const void* q, const void* k, const void* v, void* out, int32_t b,
                             int32_t s_q, int32_t s_kv, int32_t n, int32_t d, svi_stream stream);
/* Diagnostics for the long-sequence attention (keys >= 2048): one call = an optimistic pass that fixes each row's reference maximum
 * after the first key tile + a second pass in which the complete kernel recomputes exactly the workgroups whose row sums left the
 * range the fixed reference covers.  Reports, for the LAST such call enqueued on `stream`, how many workgroups were recomputed and
 * how many the launch had (drains the stream; tests use it to prove that adversarial operands take the second pass). */
svi_status svi_attention_last_flagged(svi_stream stream, int32_t* flagged_out, int32_t* workgroups_out);
/* Launch planners: pure arithmetic on sizes and the environment switches, no device work (they run on a machine without a GPU).
 * svi_gemm_plan: the kernel svi_gemm_bf16 takes for [M, K] x [N, K]^T — 0 = weight-streaming skinny kernel, 128 = 128^2 tile, 192 = 256 x 192 tile
 * (where 192-wide tiles fill the chip's rounds better: sequence-parallel shards), 259 / 260 = the 256^2 tile (four / two phases per K tile); `compute_units` = CUs of the part
 * the round arithmetic is done for (256 on MI355X; the launcher asks the device).
 * svi_attention_plan: out4 = {kernel (1 = short key axes, 2 = long-sequence kernel), work items run whole, pieces per remaining item, workgroups}:
 * the items of a partly filled last round are cut along the key axis (csrc/svi_attention.hip flash_splits). */
svi_status svi_gemm_plan(int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t skinny, int32_t compute_units, int32_t* kernel_out);
/* svi_gemm_w8_plan: the kernel svi_gemm_bf16_w8 takes for the same problem — svi_gemm_plan's answer where that kernel has an e4m3-weight form (0 and 128);
 * the LDS-DMA fed tiles (192 / 259 / 260) map to 128.  With SVI_GEMM_W8_256=1 (opt-in) those three map to 260 instead, the two-phase 256^2 tile reading
 * the stored bytes (the 192-wide and the four-phase schedule have no e4m3 twin); everything else answers as without the switch. */
svi_status svi_gemm_w8_plan(int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t skinny, int32_t compute_units, int32_t* kernel_out);
svi_status svi_attention_plan(int32_t s_q, int32_t s_kv, int32_t heads, int32_t compute_units, int32_t* out4);
/* ABI v11 — the VAE's plane-fed residual-block convolution (3x3x3 over Cin -> Cout, stride 1, causal, 'same'; input [frames][Ho][Wo][Cin]):
 * svi_vae_conv_plan: out8 = {kernel (0 = the layer does not take the producer's fp16 planes, 1 = conv_dma2h_kernel<1> (Cout <= 32), 3 = conv_dma2h_kernel<3>,
 *   2 = conv_dma2h_pair_kernel: two 256-pixel tiles per workgroup), the tile order ord_T, ord_Lf, ord_G (frames x tiles per frame walked in groups of ord_G
 *   tiles through all frames; ord_T = 0: pixel order), workgroups, the largest frame distance between the two tiles of one workgroup, the bytes the largest
 *   activation descriptor must address (must stay below 0xFFE00000), the launch guard's bound on that ((kt + 3) frames)}.  Follows SVI_VAE_PAIR,
 *   SVI_VAE_TILE_ORDER, SVI_VAE_DMA, SVI_VAE_X2H and SVI_VAE_EXACT_FP32 as the launcher does.
 * svi_vae_tile_order: out[i] (ord_T x ord_Lf entries) = the frame-major pixel tile that launch position i computes under that order. */
svi_status svi_vae_conv_plan(int32_t Cin, int32_t Cout, int32_t kt, int32_t frames, int32_t Ho, int32_t Wo, int64_t* out8);
svi_status svi_vae_tile_order(int32_t ord_T, int32_t ord_Lf, int32_t ord_G, int64_t* out);

/* nn.LayerNorm(eps) [+ affine w,b] [+ modulate(x, shift, scale)] over rows of x[rows, dim]
 * (models/wan_video_dit.py:150-151,331-333,358,372).  w,b,shift,scale are bf16 [dim] or NULL. */
svi_status svi_layernorm_modulate(const void* x, void* out, int32_t rows, int32_t dim, float eps,
                                  const void* w, const void* b, const void* shift, const void* scale,
                                  svi_stream stream);

/* RMSNorm over the full model dim, then (optionally) 3-D RoPE per head, in place on x[rows, ld]
 * (models/wan_video_dit.py:186-197 then :178-183).  grid f*h*w must equal rows when rope != 0. */
svi_status svi_rmsnorm_rope(void* x, int32_t ld, int32_t rows, int32_t dim, const void* weight, float eps,
                            int32_t rope, int32_t num_heads, int32_t f, int32_t h, int32_t w,
                            svi_stream stream);

/* ABI v12 — the q | k normalisation as the DiT block launches it before every self-attention, in place on x[rows, ld]: operand q at columns [0, dim) with
 * gain weight_q and output scale out_scale_q; with weight_k != NULL a second operand at columns [dim, 2 dim) (ld >= 2 dim) with weight_k / out_scale_k in
 * the same launch.  The output scale multiplies the result before its single final rounding (the DiT folds softmax_scale * log2(e) into q there).
 * rope: 0 none (f, h, w, row0, period ignored); 1 rotation pairs looked up in the three axis tables; 2 read from a per-token table gathered from them
 * first — the form the DiT runs, and at dim 1536 / 5120 the four-rows-per-wave kernel.  Row i is token row0 + i of the (f, h, w) grid (a sequence-parallel
 * shard starts mid-grid), or with period > 0 token row0 + i % period (samples of `period` rows stacked one under the other: the CFG pair).  Refused:
 * dim > 8192, dim or ld not a multiple of 8, RoPE with dim % 128 != 0, a grid that does not hold [row0, row0 + rows) (with period: [row0, row0 + period),
 * and rows must be a multiple of period), weight_k with ld < 2 dim.  The sequence-parallel send layout and the e4m3 output form are not reachable here. */
svi_status svi_rmsnorm_rope_qk(void* x, int32_t ld, int32_t rows, int32_t dim, const void* weight_q, const void* weight_k,
                               float eps, float out_scale_q, float out_scale_k, int32_t rope,
                               int32_t f, int32_t h, int32_t w, int32_t row0, int32_t period, svi_stream stream);

/* C[M,N] = epilogue(A[M,K] · W[N,K]^T)  — nn.Linear with the weight in its native [out,in] layout.
 * bias bf16 [N] (or [M] when bias_along_m, used to emit V^T); gate f32 [N] or NULL; res bf16 [M,ldres]
 * (may alias C).  K multiple of 8; lda/ldw/ldc multiples of 8 elements. */
svi_status svi_gemm_bf16(const void* A, int32_t lda, const void* W, int32_t ldw, void* C, int32_t ldc,
                         int32_t M, int32_t N, int32_t K, const void* bias, int32_t bias_along_m,
                         int32_t epilogue, const float* gate, const void* res, int32_t ldres,
                         svi_stream stream);
/* ABI v13 — the same GEMM as the DiT block launches it for q | k and for the stacked CFG pair: svi_gemm_bf16's arguments plus
 *   W2, bias2, n_split   two weight matrices side by side in the output: columns [0, n_split) come from W [n_split, ldw] and bias, columns [n_split, N)
 *                        from W2 [N - n_split, ldw] and bias2 (bf16 [N - n_split] or NULL).  gate, res and C span all N columns.  One launch when
 *                        n_split is a multiple of the tile width of the kernel that runs (128, 192 or 256), else one launch per matrix — the same bits
 *                        either way, and the same as two svi_gemm_bf16 calls on the halves.  W2 NULL: one matrix, n_split and bias2 ignored.
 *                        Refused: n_split <= 0 or >= N, n_split not a multiple of 8, bias_along_m with W2.
 *   sel_m, sel_n         > 0: choose the kernel as svi_gemm_plan would for a problem of sel_m rows / sel_n columns (samples stacked along M or N keep the
 *                        kernel of a per-sample launch); 0: by M / N. */
svi_status svi_gemm_bf16_pair(const void* A, int32_t lda, const void* W, int32_t ldw, void* C, int32_t ldc,
                              int32_t M, int32_t N, int32_t K, const void* bias, int32_t bias_along_m,
                              int32_t epilogue, const float* gate, const void* res, int32_t ldres,
                              const void* W2, const void* bias2, int32_t n_split, int32_t sel_m, int32_t sel_n,
                              svi_stream stream);
/* The weight-streaming skinny kernel (plan id 0: M <= 128 rows against a large weight, K % 128 == 0, epilogue SVI_EPI_BIAS or SVI_EPI_BIAS_GATE_RES, ldc % 4 == 0
 * — the text encoder's projections) as an operator seam.  w8 = 0: W bf16 [N, ldw]; w8 != 0: W stored as e4m3 bytes [N, ldw bytes], widened in front of the
 * matrix instruction — bit-identical to w8 = 0 on the widened copy.  Refused when the shape does not take that kernel. */
svi_status svi_gemm_bf16_skinny(const void* A, int32_t lda, const void* W, int32_t ldw, void* C, int32_t ldc, int32_t M, int32_t N, int32_t K,
                                const void* bias, int32_t epilogue, const float* gate, const void* res, int32_t ldres, int32_t w8, svi_stream stream);
/* FP8-resident weights: svi_gemm_bf16_pair with W (and W2) stored as OCP e4m3fn BYTES, [N, ldw] with ldw in bytes, a multiple of 16 (W / W2 16-byte aligned):
 *     C = epi(A[M, K] bf16 · widen(W8[N, K])^T)
 * The bytes are widened to bf16 (exactly: all 256 codes, subnormals m * 2^-9, signed zeros, S.1111.111 = NaN — svi_fp8_e4m3_to_bf16's mapping) between the
 * global load and the matrix instruction, so per output element the sums and their order are those of svi_gemm_bf16_pair on the widened copy run on the
 * kernel svi_gemm_w8_plan names: bit-identical, at half the weight bytes from HBM.  Every epilogue, W2 / n_split, sel_m / sel_n and bias_along_m as there.
 * Refused with a message, before any launch: a NULL A / W / C, an ldw that is not a multiple of 16. */
svi_status svi_gemm_bf16_w8(const void* A, int32_t lda, const void* W8, int32_t ldw, void* C, int32_t ldc,
                            int32_t M, int32_t N, int32_t K, const void* bias, int32_t bias_along_m,
                            int32_t epilogue, const float* gate, const void* res, int32_t ldres,
                            const void* W2_8, const void* bias2, int32_t n_split, int32_t sel_m, int32_t sel_n,
                            svi_stream stream);

/* ---- MX-fp8 (opt-in; north_star "bf16/fp8 MFMA").  The reference computes in bf16 and only STORES weights as float8_e4m3fn
 * (test_svi.py:337, vram_management/layers.py:65-71): what follows is arithmetic it never performs — own tolerance, own bench line.
 *   svi_mx8_quantize   x bf16 [rows, ldx] -> q e4m3 [rows, ldq] (OCP e4m3fn, round-to-nearest-even, saturating) with one E8M0 scale per
 *                      32 consecutive K elements (OCP MX: 2^(floor(log2 amax) - 8)); scales as dwords [K/128][sc_rows], byte b of dword
 *                      [kt][m] = block 4 kt + b of row m; K % 128 == 0, sc_rows >= rows.
 *   svi_gemm_mx8       C[M,N] = epilogue(A8[M,K] · W8[N,K]^T) on v_mfma_scale_f32_32x32x64_f8f6f4: A8 with the scales above (sc_rows a
 *                      multiple of 256 covering M), W8 e4m3 with unit scales (the reference's stored bytes); bias / epilogue / gate / res
 *                      as svi_gemm_bf16; lda / ldw in bytes, multiples of 16.
 *   svi_dit_bind_ffn_fp8 / svi_dit_ffn_mx8   hand blocks.<layer>.ffn.<0|2>.weight over as stored e4m3 bytes [out, in] and route both MLP
 *                      GEMMs of every block through svi_gemm_mx8 (activations quantised in front of each). */
svi_status svi_mx8_quantize(const void* x, int32_t ldx, int32_t rows, int32_t K, void* q, int32_t ldq, void* scales, int32_t sc_rows, svi_stream stream);
svi_status svi_gemm_mx8(const void* A8, int32_t lda, const void* a_scales, int32_t sc_rows, const void* W8, int32_t ldw, void* C, int32_t ldc,
                        int32_t M, int32_t N, int32_t K, const void* bias, int32_t epilogue, const float* gate, const void* res, int32_t ldres,
                        svi_stream stream);
svi_status svi_dit_bind_ffn_fp8(svi_dit* h, int32_t layer, int32_t which, const void* e4m3_weight);
svi_status svi_dit_ffn_mx8(svi_dit* h, int32_t enable);
/* ABI v10 (round 6) — the same opt-in arithmetic on the block's other six projections ("QKV/out-proj ... on bf16/fp8 MFMA" of the north star):
 *   svi_gemm_mx8_wscaled   C[M,N] = bf16(A8[M,K] · dequant(W8[N,K])^T + bias): the block scales ([K/128][sc_rows], sc_rows a multiple of 256 covering N) belong to
 *                          the W operand's rows, A carries unit scales — the transposed value projection V^T = Wv · X^T (A8 = the stored e4m3 weight, W8 = the
 *                          quantised activation rows, bias along M).
 *   svi_dit_bind_ffn_fp8   also takes which = 10 self_attn.q, 11 self_attn.k, 12 self_attn.v, 13 self_attn.o, 14 cross_attn.q, 15 cross_attn.o
 *                          (blocks.<layer>.<module>.weight as stored e4m3 bytes [out, in]).
 *   svi_dit_proj_mx8       route those six GEMMs of every block through the MX fp8 kernels (plain forwards and the stacked CFG pair; sequence-parallel shards keep
 *                          bf16): the LayerNorm output is quantised once for q, k and V^T, the attention outputs once for each output projection, the cross-attention
 *                          query's row statistic comes from the fp8 GEMM's epilogue as it does from the bf16 one.  The prompt-side K / V (context cache) stay bf16.
 *                          Needs all six weights of every block bound; own oracle and tolerance (tests/test_gpu_mx8.py), bench.py --fp8-all; never a default. */
svi_status svi_gemm_mx8_wscaled(const void* A8, int32_t lda, const void* W8, int32_t ldw, const void* w_scales, int32_t sc_rows, void* C, int32_t ldc,
                                int32_t M, int32_t N, int32_t K, const void* bias, int32_t bias_along_m, svi_stream stream);
svi_status svi_dit_proj_mx8(svi_dit* h, int32_t enable);

/* Classifier-free-guidance combine + FlowMatchScheduler.step, fused (pipelines/svi_video.py:410,420;
 * schedulers/flow_match.py:53-64):  lat += (uncond + s*(cond-uncond)) * (sigma_next - sigma), bf16,
 * rounded after every op exactly like the reference's bf16 tensor arithmetic.  uncond may be NULL
 * (cfg_scale == 1 path). */
svi_status svi_cfg_step(void* latents, const void* cond, const void* uncond, int64_t n, float cfg_scale,
                        float dsigma, svi_stream stream);

/* Three-way guidance of the talk sampler + FlowMatchScheduler.step (pipelines/svi_video_talk.py:455-461):
 *   v = uncond + s_text*(cond - drop_text) + s_audio*(drop_text - uncond);  lat += v * (sigma_next - sigma)
 * bf16, rounded after every op in the reference's evaluation order. */
svi_status svi_cfg3_step(void* latents, const void* cond, const void* uncond, const void* drop_text, int64_t n, float s_text,
                         float s_audio, float dsigma, svi_stream stream);

/* FP8 weight storage: the reference's `torch_dtype=torch.float8_e4m3fn` mode (test_svi.py:337) keeps parameters as OCP e4m3fn and
 * casts them to bf16 in front of every use (vram_management/layers.py:65-71, cast_to).  The cast is exact, so it is done once:
 * out bf16 [n] = bf16(in e4m3fn [n]); bind the result with svi_dit_bind_weight.  (svi_hip.WanDiT.bind does this for fp8 tensors; with fp8_resident=True it
 * binds the blocks' Linear weights as SVI_E4M3 instead and casts only the small rest.) */
svi_status svi_fp8_e4m3_to_bf16(const void* in, void* out, int64_t n, svi_stream stream);

/* The cast back: out e4m3fn [n] = cast(in [n]), in fp32 (SVI_F32) or bf16 (SVI_BF16, widened exactly), with the semantics of torch's
 * `tensor.to(torch.float8_e4m3fn)`: round to nearest even, subnormals down to 2^-9 (2^-10 ties to 0), NO saturation — 464 still rounds
 * to 448, anything above it and +-inf become NaN, NaN stays NaN.  What `load_models(torch_dtype=torch.float8_e4m3fn)` does to every
 * parameter (svi_hip.checkpoint.load_dit(torch_dtype=...)), and the last step of svi_lora_merge_e4m3. */
svi_status svi_f32_to_fp8_e4m3(const void* in, svi_dtype in_dtype, void* out, int64_t n, svi_stream stream);

/* LoRA merge into an FP8-stored weight, in place (GeneralLoRAFromPeft.load when the model's parameters are float8_e4m3fn,
 * models/lora.py:231-264: the computation dtype becomes fp32):
 *     w8 <- e4m3fn( fp32(w8) + alpha * mm( fp32(up), fp32(down) ) )
 * with the reference's three fp32 rounding points (product, scaling, sum) and the cast above.  w8 e4m3fn codes [out_f, in_f], contiguous,
 * 8-byte aligned; up [out_f, r]; down_t [in_f, r] = down TRANSPOSED (both operands k-contiguous, as svi_gemm_bf16 takes the bf16 merge's);
 * both operands of `dtype` (SVI_BF16, SVI_F16 or SVI_F32 — kept in that precision: bf16 on the bf16 matrix instruction, the other two
 * widened to fp32 on the fp32 one), contiguous and 16-byte aligned.  in_f % 8 == 0 and r % 8 == 0; any out_f. */
svi_status svi_lora_merge_e4m3(void* w8, int32_t out_f, int32_t in_f, const void* up, const void* down_t, svi_dtype dtype, int32_t r, float alpha,
                               svi_stream stream);

/* ------------------------------------------------------------------ measurement ----------- */
/* Per-kernel timing with HIP events recorded on the launch stream (so it measures the kernels where
 * they run, inside the caller's timed region).  Off by default; when on, every tagged launch inside
 * svi_dit_forward / svi_vae_* is bracketed by an event pair.  svi_prof_summary synchronises the
 * recorded events and writes one JSON object {"tag": {"count": n, "ms": total_ms}, ...} into buf. */
svi_status svi_prof_enable(int32_t on);
svi_status svi_prof_summary(char* buf, int64_t buflen);
/* Restrict recording to some tags: comma-separated names as svi_prof_summary prints them ("flash_self,gemm_ffn1"); NULL or "" = all (the
 * default).  Every event record is a packet between two kernels of the stream it measures (~1440 per C2 step with all tags, ~1 % of the
 * step); bench.py records the dominant kernel alone over its timed region and takes the full breakdown in a short pass behind it. */
svi_status svi_prof_select(const char* tags);

/* ------------------------------------------------------------------ VAE ------------------- */
/* WanVideoVAE() (models/wan_video_vae.py:599-618): fixed architecture (dim 96, z 16, mult 1,2,4,4). */
svi_status svi_vae_create(svi_vae** out);
svi_status svi_vae_destroy(svi_vae* h);
/* name = reference state-dict key ("model.decoder.conv1.weight", ...); dtype SVI_F32
 * (the pipelines run the VAE in fp32: pipelines/svi_video.py:386-387,303-309).  Convolution weights are re-packed for the
 * kernels at bind time by a launch on the NULL stream: the tensor must be complete with respect to that stream when it is
 * bound; the first encode / decode after a bind waits for the packing before it enqueues on the caller's stream. */
svi_status svi_vae_bind_weight(svi_vae* h, const char* name, const void* dev_ptr, svi_dtype dtype,
                               const int64_t* shape, int32_t rank);
svi_status svi_vae_check_bound(svi_vae* h);
/* The 8-bit frame hand-off between the clips of a stream, on the device.
 * svi_video_to_u8: SVIVideoPipeline.tensor2video (pipelines/svi_video.py:366-370): video f32 [3, T, H, W] in [-1, 1] ->
 *   frames u8 [T, H, W, 3] = uint8(clip((x + 1) * 127.5, 0, 255)).
 * svi_u8_to_video: BasePipeline.preprocess_image (pipelines/base.py:44-45): frames u8 [n, H, W, 3] -> f32 [n, 3, H, W] =
 *   float32(x) * (2 / 255) - 1.  Both bit-identical to the reference's host arithmetic. */
svi_status svi_video_to_u8(const float* video, uint8_t* frames, int32_t T, int32_t H, int32_t W, svi_stream stream);
svi_status svi_u8_to_video(const uint8_t* frames, float* video, int32_t n, int32_t H, int32_t W, svi_stream stream);

/* WanVideoVAE.decode -> single_decode -> VideoVAE_.decode (models/wan_video_vae.py:777-789,753-756,552-575)
 *   latents f32 [16, T, h, w]  ->  video f32 [3, 1+4(T-1), 8h, 8w], clamped to [-1,1]. */
svi_status svi_vae_decode(svi_vae* h, const float* latents, float* video, int32_t T, int32_t hh, int32_t ww,
                          svi_stream stream);
/* WanVideoVAE.encode -> single_encode -> VideoVAE_.encode (models/wan_video_vae.py:759-774,747-750,525-550)
 *   video f32 [3, 1+4k, H, W]  ->  latents f32 [16, 1+k, H/8, W/8]  (normalised mean). */
svi_status svi_vae_encode(svi_vae* h, const float* video, float* latents, int32_t T, int32_t H, int32_t W,
                          svi_stream stream);

/* WanVideoVAE.tiled_decode / tiled_encode (models/wan_video_vae.py:643-693 / :696-744, masks :621-640): the spatial tiling the
 * pipelines switch on with `tiled=True` (the default of SVIVideoPipeline.__call__, pipelines/svi_video.py:439).  Tiles start every
 * tile_stride, are clipped at the far edge, and a start is dropped once the previous tile reaches the edge; each tile is read in
 * place from the caller's tensor, run through the same graph as svi_vae_decode / _encode, multiplied by the linear-ramp mask
 * (ramp width = (tile_size - tile_stride), in output elements) and accumulated in task order; the result is values / weight,
 * clamped to [-1,1] for decode only AFTER the blend (tile values are not clamped, as in the reference).  `video` / `latents` serve
 * as the accumulator.  Decode: sizes and strides in LATENT pixels; encode: in VIDEO pixels, multiples of 8 (the reference's
 * encode() multiplies its latent-unit arguments by 8 before the call, :765-767). */
svi_status svi_vae_tiled_decode(svi_vae* h, const float* latents, float* video, int32_t T, int32_t hh, int32_t ww,
                                int32_t size_h, int32_t size_w, int32_t stride_h, int32_t stride_w, svi_stream stream);
svi_status svi_vae_tiled_encode(svi_vae* h, const float* video, float* latents, int32_t T, int32_t H, int32_t W,
                                int32_t size_h, int32_t size_w, int32_t stride_h, int32_t stride_w, svi_stream stream);

/* Exact spatial split of the decode, for the multi-GPU latency modes: the decoder's middle block attends over a whole frame, everything behind it
 * is local, so a part runs conv2 / conv1 / middle on the whole latent frame, crops the activation to its owned rectangle plus a halo, and runs the
 * four upsampling stages and the head on the crop, trimming the crop again after every upsample block.  Unlike the blended tiling this computes
 * what svi_vae_decode computes (up to the summation order of whichever convolution kernel a cropped shape selects).
 * svi_vae_split_plan (host arithmetic, no device): part = i * parts_w + j of a parts_h x parts_w split of the hh x ww latent grid; cuts sit at
 *   floor(i hh / parts_h), floor(j ww / parts_w).  out24 = {owned latent rectangle h0, h1, w0, w1 | halo per side entering stages 0-3, in pixels of
 *   that stage's resolution (latent x 1, 2, 4, 8), derived from the decoder's layer table | the rectangle entering stage 0 (h0, h1, w0, w1, stage
 *   resolution) | stage 1 | stage 2 | stage 3}: the owned rectangle scaled, grown by the halo along the dimensions that are cut, clamped at the
 *   image border (where the kernels' zero padding is the real padding).  A 1 x 1 split reports zero halos.
 * svi_vae_decode_part: latents f32 [16, T, hh, ww] (whole) -> the part's owned pixels of the clamped video.  `video` points at where the owned
 *   window's first pixel (channel 0, frame 0) goes; pixel (c, t, y, x) of the window is written at ((c T' + t) video_ld_h + y) video_ld_w + x,
 *   T' = 1 + 4 (T - 1).  A full frame: video_ld_h = 8 hh, video_ld_w = 8 ww and `video` offset to the window; a tight buffer: the window's own
 *   size.  Nothing else is written.  A 1 x 1 split into a full frame is svi_vae_decode.
 * svi_vae_decode_planned: the same with the caller's plan (svi_vae_split_plan's layout; the halo entries are not read).  The rectangles are held
 *   to what keeps every crop inside its tensor, not to the halo: a plan with a short halo decodes with errors next to the cuts. */
svi_status svi_vae_split_plan(int32_t hh, int32_t ww, int32_t parts_h, int32_t parts_w, int32_t part, int32_t* out24);
svi_status svi_vae_decode_part(svi_vae* h, const float* latents, float* video, int32_t T, int32_t hh, int32_t ww, int32_t parts_h, int32_t parts_w,
                               int32_t part, int32_t video_ld_h, int32_t video_ld_w, svi_stream stream);
svi_status svi_vae_decode_planned(svi_vae* h, const float* latents, float* video, int32_t T, int32_t hh, int32_t ww, const int32_t* plan24,
                                  int32_t video_ld_h, int32_t video_ld_w, svi_stream stream);

/* Exact spatial split of the encode, the decode split run the other way round: everything in front of the encoder's middle block is local, so a
 * part runs conv1 and the four down stages on a crop of the video and writes its owned rectangle of the feature map entering middle.0; one
 * all-gather assembles that map, and the middle block, the head and model.conv1 (svi_vae_encode_tail) run on the whole frame on every rank.
 * svi_vae_encode_split_plan (host arithmetic, no device): part = i * parts_w + j of a parts_h x parts_w split of the hh x ww latent grid, cut as
 *   svi_vae_split_plan cuts it.  There are five entry points: the video and the entries of stages 0-3, at 8, 8, 4, 2 and 1 pixels per latent
 *   pixel.  out34 = {owned latent rectangle h0, h1, w0, w1 | reach (top/left, bottom/right) at the five entry points, derived from the encoder's
 *   layer table | the rectangle (h0, h1, w0, w1) the part needs at the five entry points}: the owned rectangle scaled, grown by the reach, its
 *   origin rounded down to a multiple of the entry point's factor (which keeps the phase of every stride-2 convolution behind it), clamped at the
 *   image border (where the kernels' zero padding, the asymmetric right/bottom one included, is the real padding).  A 1 x 1 split reports no reach.
 * svi_vae_encode_part: video f32 [3, T, H, W] (whole; the part's window is read in place) -> the part's owned window of the feature map,
 *   channels-last f32 [T', h, w, C] (T' = 1 + (T - 1) / 4, C = the middle block's channels, 384).  `feat_out` (16-byte aligned) points at where the
 *   window's first pixel goes; pixel (t, y, x) of the window is written at ((t ld_h + y) ld_w + x) C.  A full map: ld_h = H / 8, ld_w = W / 8 and
 *   `feat_out` offset to the window; a tight buffer: the window's own size.  Nothing else is written.
 * svi_vae_encode_planned: the same with the caller's plan (svi_vae_encode_split_plan's layout; the reach entries are not read).  The rectangles
 *   are held to what keeps every window inside its tensor (and to even origins in front of the stride-2 convolutions), not to the reach: a plan
 *   with a short halo encodes with errors next to the cuts.
 * svi_vae_encode_tail: feat f32 [T', hh, ww, C] (tight) -> latents [16, T', hh, ww]: middle.0/1/2, head.0, head.2, model.conv1 and the latent
 *   normalisation, the same code svi_vae_encode runs behind its down stages. */
svi_status svi_vae_encode_split_plan(int32_t hh, int32_t ww, int32_t parts_h, int32_t parts_w, int32_t part, int32_t* out34);
svi_status svi_vae_encode_part(svi_vae* h, const float* video, float* feat_out, int32_t T, int32_t H, int32_t W, int32_t parts_h, int32_t parts_w,
                               int32_t part, int32_t ld_h, int32_t ld_w, svi_stream stream);
svi_status svi_vae_encode_planned(svi_vae* h, const float* video, float* feat_out, int32_t T, int32_t H, int32_t W, const int32_t* plan34,
                                  int32_t ld_h, int32_t ld_w, svi_stream stream);
svi_status svi_vae_encode_tail(svi_vae* h, const float* feat, float* latents, int32_t Tl, int32_t hh, int32_t ww, svi_stream stream);

/* ------------------------------------------------------------------ dance variant: pose embedder ------- */
/* The `dwpose_embedding` of SVIDanceVideoPipeline (pipelines/svi_video_dance.py:255-269): seven fp32 Conv3d layers with SiLU between
 * them, 3 -> hidden (16) channels at full resolution down to dim channels at the DiT's token grid.  svi_pose_forward also does what
 * :527-530 does around it: the pose video's first frame is repeated three more times in front, values are divided by 255, the result
 * is cast to bf16 and laid out 'b c f h w -> b (f h w) c' — exactly the `add_condition` input of svi_dit_forward (:423, :103-104).
 *   pose  f32 [3, F, H, W] (values 0..255)   ->   out bf16 [f*h*w, dim],  (f, h, w) from svi_pose_tokens (F = 81, 480x832: 21, 30, 52)
 * Weight names are the nn.Sequential's state-dict keys "0.weight", "0.bias", "2.weight", ... "12.bias" (fp32). */
typedef struct svi_pose svi_pose;
svi_status svi_pose_create(int32_t hidden, int32_t dim, svi_pose** out);
svi_status svi_pose_destroy(svi_pose* h);
svi_status svi_pose_bind_weight(svi_pose* h, const char* name, const void* dev_ptr, svi_dtype dtype, const int64_t* shape, int32_t rank);
svi_status svi_pose_check_bound(svi_pose* h);
svi_status svi_pose_tokens(svi_pose* h, int32_t F, int32_t H, int32_t W, int32_t* f, int32_t* hh, int32_t* ww);
svi_status svi_pose_forward(svi_pose* h, const float* pose, void* out, int32_t F, int32_t H, int32_t W, svi_stream stream);
/* The clip boundary of a dance STREAM (additive in v13): clip k's pose window cut on the device out of the whole pose video.
 *
 * svi_pose_window: pose u8 [N, h, w, 3] — the pose video as the video reader hands it over, at its source resolution — is read for clip k of a
 * stream whose clips have F frames and hand m motion frames from clip to clip; out f32 [3, F, H, W], values 0..255, is svi_pose_forward's input.
 * This is what the reference's script does between two clips on the host (test_svi_dance.py:215-227, 281-288 around
 * utils/image_process.py:134-170 resize_and_pad_to_target), with F where the script hard-codes 81:
 *   Frame.  Window frame i of clip k: while k > 0 and i < m, it is frame F - m + i of clip k - 1 (the carried motion poses; i and k step back until
 *     the frame is one a clip read for itself).  Then g = i when k == 0, else g = (F - 1) + (k - 1)(F - m) + (i - m): the script's read cursor starts
 *     clip 1 at F - 1, so frame F - 1 is read twice (its quirk), and runs on over the clips.  The source frame is g mod N: the wrap of the cursor, and
 *     also the repeat-padding of a video shorter than a clip (the padded length is a multiple of N).  The script's `stride` is read and never
 *     applied; nor is it here.
 *   Size.  s = min(H / h, W / w) in double; nh = (int)(h * s), nw = (int)(w * s), truncated (so nh can be H - 1 where h * (H / h) lands just under
 *     H); pad_top = (H - nh) / 2, pad_left = (W - nw) / 2, integer division: the odd pixel goes to the bottom / right.
 *   Row and column.  Output row y in [pad_top, pad_top + nh) reads source row min((int)floorf((y - pad_top) * rs), h - 1), rs = (float)h / (float)nh
 *     in fp32 — F.interpolate(mode='nearest') with the output size given.  Columns alike with w, nw, pad_left.  Everything outside is 0.
 * One launch; no host table, no allocation, no copy: the scalars are the kernel's arguments.  A lane owns four neighbouring columns of one output row
 * in all three channels (the three bytes of a source pixel are read together) and writes one 16-byte store per channel when W % 4 == 0 and out is
 * 16-byte aligned (4-byte stores otherwise); the padding is written as zeros by the same launch.  Source offsets are 64-bit (N * h * w * 3 passes
 * 2^31 for an ordinary video); F <= 65535 and H * W < 2^31.
 *
 * svi_pose_window_plan: the same rule on the host, no device touched: frame_src[F] (source frame of every window frame), row_src[H] and col_src[W]
 * (source row / column, -1 where the output is padding).  The kernel and the plan call the same inline functions.
 *
 * Both refuse, with a message and before any launch: a NULL pointer, N < 1, F < 2, m < 1 or m >= F, k < 0, h or w < 1, H or W < 16, nh or nw < 1. */
svi_status svi_pose_window(const uint8_t* pose, float* out, int32_t N, int32_t h, int32_t w, int32_t H, int32_t W, int32_t F, int32_t m, int32_t k,
                           svi_stream stream);
svi_status svi_pose_window_plan(int32_t N, int32_t h, int32_t w, int32_t H, int32_t W, int32_t F, int32_t m, int32_t k, int32_t* frame_src,
                                int32_t* row_src, int32_t* col_src);

/* ------------------------------------------------------------------ prompt-side encoders ------- */
/* WanTextEncoder (models/wan_video_text_encoder.py:209-256): the umT5 encoder behind WanPrompter.encode_prompt
 * (prompters/wan_prompter.py:99-112), bf16 as the pipeline keeps it.  Per block: T5LayerNorm, attention WITHOUT the 1/sqrt(d) scale and
 * with a relative-position bias (per layer unless shared_pos), gated-GELU feed-forward; dropout is the identity (eval).
 * Weight names are the module's state-dict keys ("token_embedding.weight", "blocks.<i>.attn.q.weight", "blocks.<i>.ffn.gate.0.weight",
 * "blocks.<i>.pos_embedding.embedding.weight", "norm.weight", ...), bf16, borrowed.
 *   svi_t5_forward: ids int64 [L] (device); the reference's mask is the tokenizer's prefix mask, given as n_valid = mask.sum():
 *   keys = positions < n_valid.  Query rows < `rows` (n_valid <= rows <= L) are computed, the rest of out bf16 [L, dim] is zero:
 *   rows = L reproduces text_encoder(ids, mask); rows = n_valid reproduces encode_prompt (it zeroes rows >= n_valid, :110-111).
 *   svi_t5_relative_buckets: host-only; T5RelativeEmbedding._relative_position_bucket (:175-194, bidirectional) for
 *   rel = key - query in -(len-1) .. len-1, out[rel + len - 1], in the host's fp32 arithmetic (what the module computes on a CPU).
 *   svi_t5_device_buckets: the table svi_t5_forward actually uses — the same function evaluated on the device in the arithmetic
 *   the module's tensor ops perform THERE (scalar division = multiplication by the fp32 reciprocal, device logf): the two can differ
 *   where the log ratio is an exact integer (|rel| = 16, 32, 64).  Copied to the host for inspection. */
typedef struct svi_t5_config {
    int32_t vocab, dim, dim_attn, dim_ffn, num_heads, num_layers, num_buckets, max_dist, shared_pos;
} svi_t5_config;
typedef struct svi_t5 svi_t5;
svi_status svi_t5_create(const svi_t5_config* cfg, svi_t5** out);
svi_status svi_t5_destroy(svi_t5* h);
svi_status svi_t5_bind_weight(svi_t5* h, const char* name, const void* dev_ptr, svi_dtype dtype, const int64_t* shape, int32_t rank);
svi_status svi_t5_check_bound(svi_t5* h);
svi_status svi_t5_forward(svi_t5* h, const int64_t* ids, int32_t L, int32_t n_valid, int32_t rows, void* out, svi_stream stream);
svi_status svi_t5_relative_buckets(int32_t num_buckets, int32_t max_dist, int32_t len, int32_t* out);
svi_status svi_t5_device_buckets(svi_t5* h, int32_t len, int32_t* out);

/* WanImageEncoder.encode_image (models/wan_video_image_encoder.py:864-880): bicubic resize to image_size^2 (align_corners=False),
 * v*0.5+0.5, CLIP mean/std normalisation, then VisionTransformer.forward(use_31_block=True) (:456-478): bias-free patch embedding,
 * class token, positional embedding, pre_norm, and the first layers_used (= num_layers - 1) pre-norm blocks (fused qkv, softmax
 * attention with 1/sqrt(d), exact GELU MLP).  fp32 throughout, as SVI runs this module (pipelines/svi_video.py:307-309) — on the exact
 * fp32 MFMA kernel.  Weight names are VisionTransformer's state-dict keys (WanImageEncoder's "model.visual." prefix stripped), fp32,
 * borrowed; post_norm.*, head and blocks >= layers_used are accepted and ignored.
 *   images f32 [B, 3, H, W] in [-1, 1]  ->  out f32 [B, tokens, dim]   (tokens = (image_size/patch_size)^2 + 1: 257 x 1280 for ViT-H/14) */
typedef struct svi_clip_config {
    int32_t image_size, patch_size, dim, mlp_ratio, num_heads, num_layers, layers_used;
    float norm_eps;
} svi_clip_config;
typedef struct svi_clip svi_clip;
svi_status svi_clip_create(const svi_clip_config* cfg, svi_clip** out);
svi_status svi_clip_destroy(svi_clip* h);
svi_status svi_clip_bind_weight(svi_clip* h, const char* name, const void* dev_ptr, svi_dtype dtype, const int64_t* shape, int32_t rank);
svi_status svi_clip_check_bound(svi_clip* h);
svi_status svi_clip_tokens(svi_clip* h, int32_t* tokens, int32_t* dim);
svi_status svi_clip_encode_image(svi_clip* h, const float* images, int32_t B, int32_t H, int32_t W, float* out, svi_stream stream);

/* The talk variant's audio encoder: wav2vec2-base (chinese-wav2vec2-base) as utils/audio_process.py:18-41 get_embedding runs it around
 * utils/src/audio_analysis/wav2vec2.py Wav2Vec2Model.forward(input_values, seq_len, output_hidden_states=True), fp32 throughout (the reference
 * runs it in fp32 on the CPU).  Waveform normalisation to zero mean / unit variance; seven bias-free Conv1d (kernels 10,3,3,3,3,2,2, strides
 * 5,2,2,2,2,2,2) with GroupNorm(C, C) after the first and exact GELU after each; linear interpolation to seq_len frames (align_corners=True);
 * LayerNorm + Linear; x + GELU(grouped positional Conv1d, padding k/2, last sample of an even kernel dropped); LayerNorm; num_layers post-norm
 * blocks.  Weight names are the Hugging Face Wav2Vec2Model's state-dict keys, fp32, borrowed; the positional convolution's weight norm is folded
 * by the caller into "encoder.pos_conv_embed.conv.weight" [hidden, hidden / pos_groups, pos_kernel]; "masked_spec_embed" is accepted and ignored.
 *   svi_w2v_frames: host-only; frames the convolution stack makes of n_samples samples (0: fewer than its 400-sample receptive field).
 *   svi_w2v_forward: samples f32 [n_samples] on the device (16 kHz mono, loudness-normalised by the caller), seq_len = int(n_samples / 16000 * 25)
 *     -> out [seq_len, num_layers, hidden] fp32 or bf16 (out_dtype): block l's output at frame t in out[t][l] — what WanDiT's audio windows are
 *     cut from.  Refused with a message, before anything runs: seq_len above the handle's frame limit (2048, the resident encoder attention's key
 *     count and about 81 s of audio, until svi_w2v_set_max_frames raises it), seq_len < 1,
 *     n_samples < 1 or below the receptive field, an unbound weight.  svi_w2v_create refuses a head size the encoder attention does not have.
 *   svi_w2v_forward_stage: the same forward up to one intermediate tensor, copied to out (f32, capacity values) — 0: normalised waveform [n];
 *     1..7: convolution layer output [frames_i, conv_dim]; 8: interpolated [seq_len, conv_dim]; 9: feature projection [seq_len, hidden];
 *     10: the positional convolution's own output; 11: the encoder's first LayerNorm; 12 + l: block l.  For tests and inspection. */
typedef struct svi_w2v_config {
    int32_t conv_dim, hidden, ffn, num_heads, num_layers, pos_kernel, pos_groups;
    float eps;
} svi_w2v_config;
typedef struct svi_w2v svi_w2v;
svi_status svi_w2v_create(const svi_w2v_config* cfg, svi_w2v** out);
svi_status svi_w2v_destroy(svi_w2v* h);
svi_status svi_w2v_bind_weight(svi_w2v* h, const char* name, const void* dev_ptr, svi_dtype dtype, const int64_t* shape, int32_t rank);
svi_status svi_w2v_check_bound(svi_w2v* h);
svi_status svi_w2v_frames(int64_t n_samples, int64_t* out);
svi_status svi_w2v_forward(svi_w2v* h, const float* samples, int64_t n_samples, int32_t seq_len, void* out, svi_dtype out_dtype, svi_stream stream);
svi_status svi_w2v_forward_stage(svi_w2v* h, const float* samples, int64_t n_samples, int32_t seq_len, int32_t stage, float* out, int64_t capacity,
                                 svi_stream stream);
/* Audio longer than 81 s (additive in ABI v13).  The reference encodes a file in ONE call, so a long file cannot be encoded in pieces.
 *   svi_w2v_set_max_frames: the handle's per-call frame limit, 2048 when the handle is made; 1 .. 65536 (43.7 min at 25 frames per second), anything
 *     else is refused with a message.  svi_w2v_forward and svi_w2v_forward_stage refuse a seq_len above the handle's limit (the message names the limit;
 *     a handle at 2048 keeps the message above and names this call).  Up to 2048 frames the forward launches exactly what it launched before, bit for
 *     bit, whatever the limit; above, its attention is the streaming kernel.  Also refused: a sample count or seq_len at which a launch with one thread
 *     per value would pass 2^32 - 256 values (frames_1 * conv_dim; seq_len * max(conv_dim, hidden, ffn)) — 41 943 044 samples at conv_dim 512.
 *   svi_encoder_attention_f32: the audio encoder's attention as an operator, O = softmax(scale Q K^T) V per head, fp32 operands on the device with
 *     leading dimensions (floats between rows; head h is columns h D .. h D + D - 1), no bias table.  kernel 0: what the audio encoder launches
 *     (resident up to 2048 keys, streaming above); 1: the resident kernel (whole score rows in LDS), refuses Lk > 2048; 2: the streaming kernel
 *     (key tiles of 256, running maximum and sum, all fp32) at any Lk.  Refused with a message naming the argument, before any launch: D other than
 *     32, 64, 80, 128; a null pointer; a leading dimension below heads * D; Lq, Lk or heads below 1; Lq or Lk above 65536; another kernel. */
svi_status svi_w2v_set_max_frames(svi_w2v* h, int32_t max_frames);
svi_status svi_encoder_attention_f32(const float* Q, int32_t ldq, const float* K, int32_t ldk, const float* V, int32_t ldv, float* O, int32_t ldo,
                                     int32_t Lq, int32_t Lk, int32_t heads, int32_t D, float scale, int32_t kernel, svi_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* SVI_HIP_H */
