// svi_encoders.hip — the two prompt-side encoders of the Wan pipelines: they run once per clip, outside the step
// loop, and produce the `context` / `clip_feature` operands of the DiT.
//
//   svi_t5    WanTextEncoder (models/wan_video_text_encoder.py:209-256): umT5 encoder, bf16 as the pipeline keeps it
//             (24 x [T5LayerNorm, attention with a per-layer relative position bias and no 1/sqrt(d) scale, gated-GELU FFN]).
//   svi_clip  WanImageEncoder.encode_image (models/wan_video_image_encoder.py:864-880): bicubic resize + CLIP normalisation +
//             the first L-1 blocks of the ViT-H/14 visual tower, fp32 as SVI runs it (pipelines/svi_video.py:307-309).
//
// All projections go through the MFMA GEMMs of the hot path (svi_launch_gemm bf16, svi_launch_gemm_f32 exact fp32); attention, the fp32
// LayerNorm and the erf GELU are svi_encoder_kernels.hip's; what is written here are the row kernels of each encoder alone.  The weight
// tables, the handle base and the workspace lists are svi_encoder_host.h's.
//
// Design choice (T5): padded positions are masked out as KEYS by the reference and their own output rows are zeroed by the caller
// (prompters/wan_prompter.py:108-112), so only the first `rows` (>= number of valid tokens) query rows are computed; rows = L gives
// the reference's text_encoder(ids, mask) output in full.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "svi_encoder_host.h"

namespace {

// ============================================================ T5 kernels ==========================================================
// token_embedding (t5:240): rows of the table
__global__ void t5_embed_kernel(const int64_t* __restrict__ ids, const bf16* __restrict__ table, bf16* __restrict__ x, int rows, int dim, int vocab) {
    const int r = blockIdx.x;
    if (r >= rows) return;
    int64_t id = ids[r];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);          // the host wrapper rejects out-of-range ids; never read outside the table
    const bf16x8* src = reinterpret_cast<const bf16x8*>(table + (size_t)id * dim);
    bf16x8* dst = reinterpret_cast<bf16x8*>(x + (size_t)r * dim);
    for (int i = threadIdx.x; i < dim / 8; i += blockDim.x) dst[i] = src[i];
}

// T5LayerNorm in a bf16 module (t5:31-35): bf16( w * bf16( x * rsqrt(mean(x^2) + eps) ) ), statistics in fp32.  One wave per row.
__global__ __launch_bounds__(256) void t5_norm_kernel(const bf16* __restrict__ x, bf16* __restrict__ out, const bf16* __restrict__ w, int rows,
                                                      int dim, float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const bf16* xp = x + (size_t)row * dim;
    float ss = 0.f;
    for (int i = lane * 8; i < dim; i += 512) {
        const bf16x8 v = ld_bf16x8(xp + i);
#pragma unroll
        for (int e = 0; e < 8; ++e) ss = fmaf((float)v[e], (float)v[e], ss);
    }
    ss = wave_sum(ss);
    const float r = rsqrtf(ss / (float)dim + eps);
    bf16* op = out + (size_t)row * dim;
    for (int i = lane * 8; i < dim; i += 512) {
        const bf16x8 v = ld_bf16x8(xp + i), ww = ld_bf16x8(w + i);
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (bf16)((float)ww[e] * rbf((float)v[e] * r));
        st_bf16x8(op + i, o);
    }
}

// fc1(x) * GELU(gate(x)) with the reference's own GELU (t5:16-20), evaluated op by op in bf16 as a bf16 module does:
//   0.5 * x * (1.0 + tanh( sqrt(2/pi) * (x + 0.044715 * pow(x, 3)) ))
__global__ void t5_gated_gelu_kernel(const bf16* __restrict__ gate, const bf16* __restrict__ fc1, bf16* __restrict__ out, long n) {
    const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
    if (i >= n) return;
    const bf16x8 g = ld_bf16x8(gate + i), f = ld_bf16x8(fc1 + i);
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float x = (float)g[e];
        const float a = rbf(0.5f * x);
        const float p = rbf(x * x * x);                     // exact in fp32 (3 x 8 significant bits), then the bf16 rounding of torch.pow
        const float b = rbf(0.044715f * p);
        const float c = rbf(x + b);
        const float d = rbf(0.7978845608028654f * c);
        const float t = rbf(tanhf(d));
        const float u = rbf(1.0f + t);
        const float ge = rbf(a * u);
        o[e] = (bf16)((float)f[e] * ge);
    }
    st_bf16x8(out + i, o);
}

__global__ void zero_bf16_kernel(bf16* __restrict__ p, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = (bf16)0.f;
}

// ============================================================ CLIP kernels ========================================================
// cubic convolution coefficients, A = -0.75 (torch upsample_bicubic2d)
__device__ __forceinline__ void cubic_coeffs(float t, float (&w)[4]) {
    const float A = -0.75f;
    const float x0 = t + 1.0f, x1 = t, x2 = 1.0f - t, x3 = x2 + 1.0f;
    w[0] = ((A * x0 - 5.0f * A) * x0 + 8.0f * A) * x0 - 4.0f * A;
    w[1] = ((A + 2.0f) * x1 - (A + 3.0f)) * x1 * x1 + 1.0f;
    w[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
    w[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
}
// encode_image preprocessing (image_encoder:866-873) fused with the patch gather of the patch-embedding convolution:
//   bicubic (align_corners=False, no antialias) [3,H,W] -> [3,S,S];  v*0.5+0.5;  (v - mean) / std;  then patch (py,px), element (c,ky,kx)
//   goes to patches[py*np + px][c*ps*ps + ky*ps + kx]  (the Conv2d weight [dim,3,ps,ps] flattened is the matching [dim, 3*ps*ps] matrix)
#pragma clang fp contract(off)
__global__ void clip_preprocess_kernel(const float* __restrict__ img, int H, int W, float* __restrict__ patches, int S, int ps, int ldp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3 * S * S) return;
    const int c = i / (S * S), oy = (i / S) % S, ox = i % S;
    const float sy = (float)H / (float)S, sx = (float)W / (float)S;
    const float ry = sy * ((float)oy + 0.5f) - 0.5f, rx = sx * ((float)ox + 0.5f) - 0.5f;
    const float fy = floorf(ry), fx = floorf(rx);
    const int iy = (int)fy, ix = (int)fx;
    float wy[4], wx[4];
    cubic_coeffs(ry - fy, wy);
    cubic_coeffs(rx - fx, wx);
    const float* src = img + (size_t)c * H * W;
    float v = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int yy = min(max(iy - 1 + a, 0), H - 1);
        float rowv = 0.f;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int xx = min(max(ix - 1 + b, 0), W - 1);
            rowv += src[(size_t)yy * W + xx] * wx[b];
        }
        v += rowv * wy[a];
    }
    const float mean[3] = {0.48145466f, 0.4578275f, 0.40821073f}, sd[3] = {0.26862954f, 0.26130258f, 0.27577711f};
    v = v * 0.5f + 0.5f;
    v = (v - mean[c]) / sd[c];
    const int np = S / ps, py = oy / ps, ky = oy - py * ps, px = ox / ps, kx = ox - px * ps;
    patches[(size_t)(py * np + px) * ldp + (c * ps + ky) * ps + kx] = v;
}
#pragma clang fp contract(fast)

// row 0 of the token matrix: cls_embedding + pos_embedding[0]  (image_encoder:460-466)
__global__ void clip_cls_kernel(const float* __restrict__ cls, const float* __restrict__ pos, float* __restrict__ x, int dim) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < dim) x[i] = cls[i] + pos[i];
}

}  // namespace

// ================================================================= T5 ==============================================================
struct svi_t5 : EncHandle {
    svi_t5_config cfg{};
    int* tab = nullptr; int tab_len = 0;            // relative-position buckets for offsets -(tab_len-1) .. tab_len-1
    int tab_host = 0;                                // built in the host's arithmetic (SVI_T5_BUCKETS=host) or the device's
};

// T5RelativeEmbedding._relative_position_bucket (t5:175-194), bidirectional, for rel = key - query, on the host in the fp32 steps of the
// reference's tensor ops.
extern "C" svi_status svi_t5_relative_buckets(int32_t num_buckets, int32_t max_dist, int32_t len, int32_t* out) {
    SVI_REQUIRE(out && num_buckets >= 4 && num_buckets % 2 == 0 && max_dist > num_buckets / 4 && len > 0, "svi_t5_relative_buckets: bad argument");
    const int nb = num_buckets / 2, max_exact = nb / 2;
    const float denom = (float)log((double)max_dist / (double)max_exact);          // math.log(...) of Python floats, then an fp32 tensor op
    for (int rel = -(len - 1); rel <= len - 1; ++rel) {
        int b = rel > 0 ? nb : 0;
        const int a = abs(rel);
        if (a < max_exact) b += a;
        else {
            const float v = logf((float)a / (float)max_exact) / denom * (float)(nb - max_exact);
            int large = max_exact + (int)v;
            if (large > nb - 1) large = nb - 1;
            b += large;
        }
        out[rel + len - 1] = b;
    }
    return SVI_OK;
}

// The same table built ON THE DEVICE, in the arithmetic the reference's tensor ops perform there: the module evaluates
// _relative_position_bucket on the embedding's device (t5:160-165), and a CUDA/HIP tensor divided by a Python scalar is multiplied
// by the scalar's fp32 reciprocal (ATen BinaryDivTrueKernel), the logarithm is the device's logf.  At offsets where the ratio is an
// exact integer (|rel| = 16, 32, 64 for the Wan configuration) the host's division and the device's reciprocal-multiply can fall on
// different sides of it, which selects a different bias row — so the table a GPU forward uses is made by the GPU's arithmetic.
__global__ void t5_bucket_kernel(int nb, int max_exact, float inv_exact, float inv_denom, float span, int len, int* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * len - 1) return;
    const int rel = i - (len - 1);
    int b = rel > 0 ? nb : 0;
    const int a = rel < 0 ? -rel : rel;
    if (a < max_exact) b += a;
    else {
        const float x = (float)a * inv_exact;              // rel_pos.float() / max_exact
        float v = logf(x) * inv_denom;                     // torch.log(.) / math.log(max_dist / max_exact)
        v = v * span;                                      // * (num_buckets - max_exact)
        long large = (long)max_exact + (long)v;            // .long() truncates toward zero
        if (large > nb - 1) large = nb - 1;
        b += (int)large;
    }
    out[i] = b;
}
static svi_status t5_device_table(svi_t5* h, int L) {
    const int want_host = svi_switches().t5_host_buckets;
    if (h->tab_len >= L && h->tab_host == want_host) return SVI_OK;
    const svi_t5_config& c = h->cfg;
    if (h->tab) { SVI_CHECK_HIP(hipFree(h->tab)); h->tab = nullptr; h->tab_len = 0; }
    SVI_CHECK_HIP(hipMalloc((void**)&h->tab, (size_t)(2 * L - 1) * 4));
    h->tab_host = want_host;
    if (want_host) {           // SVI_T5_BUCKETS=host: the CPU module's arithmetic (tests against CPU-made fixtures)
        std::vector<int32_t> host((size_t)2 * L - 1);
        SVI_TRY(svi_t5_relative_buckets(c.num_buckets, c.max_dist, L, host.data()));
        SVI_CHECK_HIP(hipMemcpy(h->tab, host.data(), host.size() * 4, hipMemcpyHostToDevice));
        SVI_CHECK_HIP(hipDeviceSynchronize());
        h->tab_len = L;
        return SVI_OK;
    }
    const int nb = c.num_buckets / 2, max_exact = nb / 2;
    const float inv_exact = 1.0f / (float)max_exact;
    const float inv_denom = 1.0f / (float)log((double)c.max_dist / (double)max_exact);
    hipLaunchKernelGGL(t5_bucket_kernel, dim3((2 * L - 1 + 255) / 256), dim3(256), 0, nullptr, nb, max_exact, inv_exact, inv_denom,
                       (float)(nb - max_exact), L, h->tab);
    SVI_LAUNCH_CHECK();
    SVI_CHECK_HIP(hipDeviceSynchronize());                  // allocation-time work on the null stream: the caller's stream need not be ordered after it
    h->tab_len = L;
    return SVI_OK;
}
// The device-built table for offsets -(len-1) .. len-1 (tests compare it with the reference formula evaluated by torch on the device).
extern "C" svi_status svi_t5_device_buckets(svi_t5* h, int32_t len, int32_t* out) {
    SVI_REQUIRE(h && out && len > 0 && len <= 2048, "svi_t5_device_buckets: bad argument");
    SVI_REQUIRE_DEVICE(h);
    SVI_TRY(t5_device_table(h, len));
    std::vector<int32_t> host((size_t)2 * h->tab_len - 1);
    SVI_CHECK_HIP(hipMemcpy(host.data(), h->tab, host.size() * 4, hipMemcpyDeviceToHost));
    for (int rel = -(len - 1); rel <= len - 1; ++rel) out[rel + len - 1] = host[(size_t)(rel + h->tab_len - 1)];
    return SVI_OK;
}

// WanTextEncoder's state dict.  The relative-position table is the module's own (shared_pos) or one per block, never both.
static const char* const T5_POS = "pos_embedding.embedding.weight";
static void t5_table(const svi_t5_config& c, EncTable* t) {
    const int64_t d = c.dim, da = c.dim_attn, df = c.dim_ffn;
    const unsigned shared = c.shared_pos ? 0 : ENC_ABSENT, per_block = c.shared_pos ? ENC_ABSENT : 0;
    t->noun = "text encoder"; t->bind_fn = "svi_t5_bind_weight"; t->max_rank = 2;
    t->dtype = SVI_BF16; t->dtype_words = "bf16 (the pipeline keeps this module in bf16)";
    t->layer_prefix = "blocks."; t->layers = t->layers_used = c.num_layers;
    t->rows = {{"token_embedding.weight", {c.vocab, d}, 0},
               {"norm.weight", {d}, 0},
               {T5_POS, {c.num_buckets, c.num_heads}, shared},
               {"norm1.weight", {d}, ENC_LAYER}, {"norm2.weight", {d}, ENC_LAYER},
               {"attn.q.weight", {da, d}, ENC_LAYER}, {"attn.k.weight", {da, d}, ENC_LAYER}, {"attn.v.weight", {da, d}, ENC_LAYER},
               {"attn.o.weight", {d, da}, ENC_LAYER},
               {"ffn.gate.0.weight", {df, d}, ENC_LAYER}, {"ffn.fc1.weight", {df, d}, ENC_LAYER}, {"ffn.fc2.weight", {d, df}, ENC_LAYER},
               {T5_POS, {c.num_buckets, c.num_heads}, ENC_LAYER | per_block}};
}

extern "C" svi_status svi_t5_create(const svi_t5_config* cfg, svi_t5** out) {
    SVI_REQUIRE(cfg && out, "svi_t5_create: null argument");
    SVI_REQUIRE(cfg->vocab > 0 && cfg->dim > 0 && cfg->dim % 8 == 0 && cfg->dim_attn > 0 && cfg->dim_attn % 8 == 0 && cfg->dim_ffn > 0 &&
                cfg->dim_ffn % 8 == 0 && cfg->num_heads > 0 && cfg->dim_attn % cfg->num_heads == 0 && cfg->num_layers > 0,
                "svi_t5_create: dim, dim_attn, dim_ffn must be positive multiples of 8 and heads must divide dim_attn");
    const int D = cfg->dim_attn / cfg->num_heads;
    SVI_REQUIRE(svi_enc_head_dim_ok(D), "svi_t5_create: head dim %d (supported: 32, 64, 80, 128)", D);
    SVI_REQUIRE(cfg->num_buckets >= 4 && cfg->num_buckets % 2 == 0 && cfg->max_dist > cfg->num_buckets / 4, "svi_t5_create: bad bucket configuration");
    svi_t5* h = new (std::nothrow) svi_t5();
    if (!h) { svi_set_error("out of host memory"); return SVI_ERR_OOM; }
    h->cfg = *cfg;
    t5_table(*cfg, &h->w);
    *out = h;
    return SVI_OK;
}

extern "C" svi_status svi_t5_destroy(svi_t5* h) {
    if (!h) return SVI_OK;
    if (h->ws) (void)hipFree(h->ws);
    if (h->tab) (void)hipFree(h->tab);
    delete h;
    return SVI_OK;
}

extern "C" svi_status svi_t5_bind_weight(svi_t5* h, const char* name, const void* dev_ptr, svi_dtype dtype, const int64_t* shape, int32_t rank) {
    SVI_REQUIRE(h, "svi_t5_bind_weight: bad argument");
    return h->w.bind(name, dev_ptr, dtype, shape, rank);
}

extern "C" svi_status svi_t5_check_bound(svi_t5* h) {
    SVI_REQUIRE(h, "null handle");
    return h->w.check_bound();
}

// ids int64 [L] on the device; keys = the first n_valid positions (the mask of the reference is a prefix mask: tokenizer padding);
// query rows 0..rows-1 are computed (n_valid <= rows <= L), the remaining rows of out [L, dim] bf16 are zero.
extern "C" svi_status svi_t5_forward(svi_t5* h, const int64_t* ids, int32_t L, int32_t n_valid, int32_t rows, void* out, svi_stream stream) {
    SVI_REQUIRE(h && ids && out, "svi_t5_forward: null argument");
    SVI_REQUIRE(L > 0 && n_valid >= 1 && n_valid <= rows && rows <= L && L <= 2048, "svi_t5_forward: need 1 <= n_valid <= rows <= L <= 2048 (got %d, %d, %d)",
                n_valid, rows, L);
    SVI_REQUIRE_DEVICE(h);
    SVI_TRY(svi_t5_check_bound(h));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const svi_t5_config& c = h->cfg;
    const int R = rows, dim = c.dim, da = c.dim_attn, df = c.dim_ffn, D = da / c.num_heads;
    SVI_TRY(t5_device_table(h, L));
    T5Bufs bufs;
    SVI_TRY(svi_enc_carve(h, [&](EncArena& a) { bufs = t5_buffers(a, R, dim, da, df); }));
    const auto [X, N, Qb, Kb, Vb, Ab, G, F1] = bufs;
#define W(k) SVI_ENC_W(bf16, h->w, k)
    auto linear = [&](const bf16* A, int K, const bf16* Wm, int Nn, bf16* Cm, const bf16* res) {
        SviGemmArgs g{};
        g.A = A; g.lda = K; g.W = Wm; g.ldw = K; g.C = Cm; g.ldc = Nn; g.M = R; g.N = Nn; g.K = K;
        g.epi = res ? SVI_EPI_BIAS_GATE_RES : SVI_EPI_BIAS;               // res: bf16(res + bf16(acc)), the module output rounded first (t5:137-138)
        g.res = res; g.ldres = Nn;
        g.skinny = 1;                                                      // taken when R <= 128 (a prompt's valid tokens), see svi_gemm.hip
        return svi_launch_gemm(g, st);
    };
    auto norm = [&](const bf16* in, bf16* o, const bf16* w) {
        hipLaunchKernelGGL(t5_norm_kernel, dim3((R + 3) / 4), dim3(256), 0, st, in, o, w, R, dim, 1e-6f);
    };
    hipLaunchKernelGGL(t5_embed_kernel, dim3(R), dim3(256), 0, st, ids, W("token_embedding.weight"), X, R, dim, c.vocab);
    SVI_LAUNCH_CHECK();
    for (int i = 0; i < c.num_layers; ++i) {
        const std::string b = "blocks." + std::to_string(i) + ".";
        norm(X, N, W(b + "norm1.weight"));
        SVI_LAUNCH_CHECK();
        SVI_TRY(linear(N, dim, W(b + "attn.q.weight"), da, Qb, nullptr));
        SVI_TRY(linear(N, dim, W(b + "attn.k.weight"), da, Kb, nullptr));
        SVI_TRY(linear(N, dim, W(b + "attn.v.weight"), da, Vb, nullptr));
        const bf16* emb = W(c.shared_pos ? std::string(T5_POS) : b + T5_POS);
        SVI_TRY(svi_launch_enc_attention_bf16(Qb, da, Kb, da, Vb, da, Ab, da, R, n_valid, c.num_heads, D, 1.0f, emb, h->tab, h->tab_len - 1, st));
        SVI_TRY(linear(Ab, da, W(b + "attn.o.weight"), dim, X, X));
        norm(X, N, W(b + "norm2.weight"));
        SVI_LAUNCH_CHECK();
        SVI_TRY(linear(N, dim, W(b + "ffn.gate.0.weight"), df, G, nullptr));
        SVI_TRY(linear(N, dim, W(b + "ffn.fc1.weight"), df, F1, nullptr));
        const long n = (long)R * df;
        hipLaunchKernelGGL(t5_gated_gelu_kernel, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, st, G, F1, G, n);
        SVI_LAUNCH_CHECK();
        SVI_TRY(linear(G, df, W(b + "ffn.fc2.weight"), dim, X, X));
    }
    hipLaunchKernelGGL(t5_norm_kernel, dim3((R + 3) / 4), dim3(256), 0, st, X, reinterpret_cast<bf16*>(out), W("norm.weight"), R, dim, 1e-6f);
    if (R < L) {
        const long n = (long)(L - R) * dim;
        hipLaunchKernelGGL(zero_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, reinterpret_cast<bf16*>(out) + (size_t)R * dim, n);
    }
    SVI_LAUNCH_CHECK();
    return SVI_OK;
#undef W
}

// ================================================================= CLIP ============================================================
struct svi_clip : EncHandle { svi_clip_config cfg{}; };

// VisionTransformer's state dict; encode_image stops after block layers_used - 1 and reads neither the last block(s), post_norm nor the head
static void clip_table(const svi_clip_config& c, EncTable* t) {
    const int64_t d = c.dim, np = (c.image_size / c.patch_size) * (c.image_size / c.patch_size), md = c.dim * c.mlp_ratio;
    t->noun = "image encoder"; t->bind_fn = "svi_clip_bind_weight"; t->max_rank = 4;
    t->dtype = SVI_F32; t->dtype_words = "fp32 (SVI runs this module in fp32)";
    t->layer_prefix = "transformer."; t->layers = c.num_layers; t->layers_used = c.layers_used;
    t->rows = {{"patch_embedding.weight", {d, 3, c.patch_size, c.patch_size}, 0},
               {"cls_embedding", {1, 1, d}, 0},
               {"pos_embedding", {1, np + 1, d}, 0},
               {"pre_norm.weight", {d}, 0}, {"pre_norm.bias", {d}, 0},
               {"post_norm.weight", {}, ENC_UNUSED}, {"post_norm.bias", {}, ENC_UNUSED}, {"head", {}, ENC_UNUSED},
               {"norm1.weight", {d}, ENC_LAYER}, {"norm1.bias", {d}, ENC_LAYER},
               {"attn.to_qkv.weight", {3 * d, d}, ENC_LAYER}, {"attn.to_qkv.bias", {3 * d}, ENC_LAYER},
               {"attn.proj.weight", {d, d}, ENC_LAYER}, {"attn.proj.bias", {d}, ENC_LAYER},
               {"norm2.weight", {d}, ENC_LAYER}, {"norm2.bias", {d}, ENC_LAYER},
               {"mlp.0.weight", {md, d}, ENC_LAYER}, {"mlp.0.bias", {md}, ENC_LAYER},
               {"mlp.2.weight", {d, md}, ENC_LAYER}, {"mlp.2.bias", {d}, ENC_LAYER}};
}

extern "C" svi_status svi_clip_create(const svi_clip_config* cfg, svi_clip** out) {
    SVI_REQUIRE(cfg && out, "svi_clip_create: null argument");
    SVI_REQUIRE(cfg->image_size > 0 && cfg->patch_size > 0 && cfg->image_size % cfg->patch_size == 0 && cfg->dim > 0 && cfg->dim % 4 == 0 &&
                cfg->num_heads > 0 && cfg->dim % cfg->num_heads == 0 && cfg->mlp_ratio > 0 && cfg->num_layers > 0 && cfg->layers_used > 0 &&
                cfg->layers_used <= cfg->num_layers && cfg->norm_eps > 0.f,
                "svi_clip_create: bad configuration (patch must divide image size, heads must divide dim, dim %% 4 == 0)");
    SVI_REQUIRE((3 * cfg->patch_size * cfg->patch_size) % 4 == 0, "svi_clip_create: 3 * patch_size^2 must be a multiple of 4");
    const int D = cfg->dim / cfg->num_heads;
    SVI_REQUIRE(svi_enc_head_dim_ok(D), "svi_clip_create: head dim %d (supported: 32, 64, 80, 128)", D);
    svi_clip* h = new (std::nothrow) svi_clip();
    if (!h) { svi_set_error("out of host memory"); return SVI_ERR_OOM; }
    h->cfg = *cfg;
    clip_table(*cfg, &h->w);
    *out = h;
    return SVI_OK;
}

extern "C" svi_status svi_clip_destroy(svi_clip* h) {
    if (!h) return SVI_OK;
    if (h->ws) (void)hipFree(h->ws);
    delete h;
    return SVI_OK;
}

// name = VisionTransformer state-dict key (the "model.visual." prefix of WanImageEncoder stripped by the caller); fp32.
extern "C" svi_status svi_clip_bind_weight(svi_clip* h, const char* name, const void* dev_ptr, svi_dtype dtype, const int64_t* shape, int32_t rank) {
    SVI_REQUIRE(h, "svi_clip_bind_weight: bad argument");
    return h->w.bind(name, dev_ptr, dtype, shape, rank);
}

extern "C" svi_status svi_clip_check_bound(svi_clip* h) {
    SVI_REQUIRE(h, "null handle");
    return h->w.check_bound();
}

extern "C" svi_status svi_clip_tokens(svi_clip* h, int32_t* tokens, int32_t* dim) {
    SVI_REQUIRE(h && tokens && dim, "svi_clip_tokens: null argument");
    const int np = h->cfg.image_size / h->cfg.patch_size;
    *tokens = np * np + 1; *dim = h->cfg.dim;
    return SVI_OK;
}

// images f32 [B, 3, H, W] in [-1, 1]  ->  out f32 [B, tokens, dim]: the hidden states after block layers_used-1
extern "C" svi_status svi_clip_encode_image(svi_clip* h, const float* images, int32_t B, int32_t H, int32_t Wd, float* out, svi_stream stream) {
    SVI_REQUIRE(h && images && out && B > 0 && H > 0 && Wd > 0, "svi_clip_encode_image: bad argument");
    SVI_REQUIRE_DEVICE(h);
    SVI_TRY(svi_clip_check_bound(h));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const svi_clip_config& c = h->cfg;
    const int S = c.image_size, ps = c.patch_size, npx = S / ps, np = npx * npx, T = np + 1, dim = c.dim, md = dim * c.mlp_ratio, D = dim / c.num_heads;
    const int kp = 3 * ps * ps;
    ClipBufs bufs;
    SVI_TRY(svi_enc_carve(h, [&](EncArena& a) { bufs = clip_buffers(a, np, kp, T, dim, md); }));
    const auto [P, X0, N, A, QKV, Hd] = bufs;
#define W(k) SVI_ENC_W(float, h->w, k)
    auto ln = [&](const float* in, float* o, const std::string& name) -> svi_status {
        return svi_launch_layernorm_f32(in, o, W(name + ".weight"), W(name + ".bias"), T, dim, c.norm_eps, st);
    };
    const float scale = 1.0f / sqrtf((float)D);
    for (int b = 0; b < B; ++b) {
        float* X = out + (size_t)b * T * dim;                        // the residual stream lives in the output
        hipLaunchKernelGGL(clip_preprocess_kernel, dim3((3 * S * S + 255) / 256), dim3(256), 0, st, images + (size_t)b * 3 * H * Wd, H, Wd, P, S, ps, kp);
        hipLaunchKernelGGL(clip_cls_kernel, dim3((dim + 255) / 256), dim3(256), 0, st, W("cls_embedding"), W("pos_embedding"), X0, dim);
        SVI_LAUNCH_CHECK();
        // patch embedding (bias-free Conv2d, stride = kernel) + positional embedding rows 1..np as the residual operand
        SVI_TRY(svi_launch_gemm_f32(P, kp, W("patch_embedding.weight"), kp, nullptr, X0 + dim, dim, np, dim, kp, W("pos_embedding") + dim, dim, st));
        SVI_TRY(ln(X0, X, "pre_norm"));
        for (int i = 0; i < c.layers_used; ++i) {
            const std::string t = "transformer." + std::to_string(i) + ".";
            SVI_TRY(ln(X, N, t + "norm1"));
            SVI_TRY(svi_launch_gemm_f32(N, dim, W(t + "attn.to_qkv.weight"), dim, W(t + "attn.to_qkv.bias"), QKV, 3 * dim, T, 3 * dim, dim, nullptr, 0, st));
            SVI_TRY(svi_launch_enc_attention_f32(QKV, 3 * dim, QKV + dim, 3 * dim, QKV + 2 * dim, 3 * dim, A, dim, T, T, c.num_heads, D, scale,
                                                 SVI_ENC_ATT_RESIDENT, st));            // the token count is the configuration's: no streaming here
            SVI_TRY(svi_launch_gemm_f32(A, dim, W(t + "attn.proj.weight"), dim, W(t + "attn.proj.bias"), X, dim, T, dim, dim, X, dim, st));
            SVI_TRY(ln(X, N, t + "norm2"));
            SVI_TRY(svi_launch_gemm_f32(N, dim, W(t + "mlp.0.weight"), dim, W(t + "mlp.0.bias"), Hd, md, T, md, dim, nullptr, 0, st));
            SVI_TRY(svi_launch_gelu_erf_f32(Hd, (long)T * md, st));
            SVI_TRY(svi_launch_gemm_f32(Hd, md, W(t + "mlp.2.weight"), md, W(t + "mlp.2.bias"), X, dim, T, dim, md, X, dim, st));
        }
    }
    return SVI_OK;
#undef W
}
