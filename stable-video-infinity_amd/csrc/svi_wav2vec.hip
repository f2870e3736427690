// svi_wav2vec.hip — the talk variant's audio encoder: wav2vec2-base as the reference runs it once per audio file
// (utils/audio_process.py:18-41 get_embedding around utils/src/audio_analysis/wav2vec2.py Wav2Vec2Model.forward), fp32 throughout as the
// reference runs it on the CPU.
//
//   waveform  -> zero mean / unit variance (Wav2Vec2FeatureExtractor)
//             -> 7 bias-free Conv1d, kernels (10,3,3,3,3,2,2), strides (5,2,2,2,2,2,2); GroupNorm(C, C) after the first; GELU after each
//             -> linear interpolation to seq_len frames (align_corners=True, torch_utils.py:16-19)
//             -> LayerNorm(C), Linear C -> H
//             -> x + GELU(grouped Conv1d(H, H, k, padding k/2) with the last sample dropped), LayerNorm
//             -> num_layers post-norm blocks: x = LN(x + attn(x)); x = LN(x + ffn(x))
//   out[t][l][:] = the output of block l at frame t  (torch.stack(hidden_states[1:], 1) rearranged "b s d -> s b d")
//
// Activations are time-major [T, C].  The projections run on the exact-fp32 MFMA GEMM; attention, LayerNorm and GELU are the fp32 launchers of
// svi_encoder_kernels.hip, the image encoder's too.  Here: one direct convolution kernel (a window of k rows of a time-major activation is k * Cin contiguous
// floats; it serves the feature extractor's layers and, with groups and a symmetric pad, the positional convolution), the statistics over time of the
// waveform and of the first layer's GroupNorm, the interpolation, and the writer of the [seq_len, layers, hidden] output.
//
// Length: the reference hands the whole file to the model in one call (every frame attends to every other, the waveform statistics are the file's), so
// a file cannot be encoded in pieces.  A handle serves up to max_frames frames per call: 2048 when it is made (the resident attention kernel's key
// count, about 81 s), up to W2V_FRAME_CAP = 65536 (43.7 min) after svi_w2v_set_max_frames.  Up to 2048 frames the attention is the resident kernel,
// above it the streaming kernel (online softmax, fp32 throughout, LDS independent of the key count); nothing else in the forward depends on the length.
#include <math.h>

#include "svi_encoder_host.h"

// This file's kernels are compiled with floating-point contraction allowed, as they always were: they used to follow the image encoder's preprocessing
// kernel, which ends with this pragma, in one translation unit.  The committed fixtures are these bits.
#pragma clang fp contract(fast)

namespace {

constexpr int W2V_CONVS = 7;
const int W2V_KERNEL[W2V_CONVS] = {10, 3, 3, 3, 3, 2, 2};
const int W2V_STRIDE[W2V_CONVS] = {5, 2, 2, 2, 2, 2, 2};
constexpr int W2V_MAX_FRAMES = 2048;              // a fresh handle's frame limit: the resident encoder attention's key limit
constexpr int W2V_FRAME_CAP = 65536;              // the most svi_w2v_set_max_frames grants (43.7 min at 25 frames per second); the audit is in DESIGN §4
static_assert(W2V_MAX_FRAMES == SVI_ENC_RESIDENT_KEYS && W2V_FRAME_CAP == SVI_ENC_MAX_KEYS, "the frame limits are the encoder attention's key limits");
constexpr long W2V_LAUNCH_ELEMS = 0xffffff00L;    // one thread per value, 256 per workgroup: the runtime launches at most 2^32 - 1 threads along x
constexpr float W2V_GROUPNORM_EPS = 1e-5f;        // nn.GroupNorm's default (the model does not pass its layer_norm_eps there)
constexpr float W2V_WAVE_EPS = 1e-7f;             // Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm

// frames after conv layer `upto` (exclusive) of n samples; <= 0: the audio is shorter than a layer's kernel
long w2v_frames_after(long n, int upto) {
    for (int i = 0; i < upto; ++i) {
        if (n < W2V_KERNEL[i]) return 0;
        n = (n - W2V_KERNEL[i]) / W2V_STRIDE[i] + 1;
    }
    return n;
}

// ---------------------------------------------------------------- direct convolution ----------------------------------------------
// y[t][g Cout_g + co] = epi( sum_{ci < Cin_g, kk < k} x[t s + kk - pad][g Cin_g + ci] * w[g Cout_g + co][ci][kk] ),  t < Tout; rows outside [0, Tin) are zero.
// w is the Conv1d weight as torch stores it, [Cout][Cin_g][k].  epi: + bias, GELU (erf), + res[t][channel], each optional, in this order.
// One workgroup = 64 frames x 64 output channels of one group; a thread owns 4 x 4 of them (frames ty + 16 i, channels tx + 16 j).  The reduction
// walks the input channels in chunks of CI (CI k <= 128 terms): a chunk's products are summed on their own and then added to the running sum, so
// the rounding error grows with the chunk count plus the chunk length, not with their product.
struct W2vConv {
    const float* x; long Tin; int ldx;
    const float* w; const float* bias; const float* res; int ldres;
    float* y; int ldy; long Tout;
    int Cin_g, Cout_g, groups, k, s, pad, CI, gelu;
};
constexpr int CV_T = 64, CV_C = 64, CV_CP = CV_C + 1;

__global__ __launch_bounds__(256) void w2v_conv1d_kernel(W2vConv a) {
    extern __shared__ __attribute__((aligned(16))) float cv_smem[];
    const int rows = (CV_T - 1) * a.s + a.k, CIp = a.CI + 1, CK = a.CI * a.k;
    float* Xs = cv_smem;                         // [rows][CIp]
    float* Ws = cv_smem + rows * CIp;            // [CK][CV_CP]
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int nct = (a.Cout_g + CV_C - 1) / CV_C, g = blockIdx.y / nct, c0 = (blockIdx.y - g * nct) * CV_C;
    const long t0 = (long)blockIdx.x * CV_T, in0 = t0 * a.s - a.pad;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int ci0 = 0; ci0 < a.Cin_g; ci0 += a.CI) {
        const int nci = min(a.CI, a.Cin_g - ci0);
        for (int i = tid; i < rows * a.CI; i += 256) {
            const int r = i / a.CI, c = i - r * a.CI;
            const long row = in0 + r;
            Xs[r * CIp + c] = (row >= 0 && row < a.Tin && c < nci) ? a.x[(size_t)row * a.ldx + g * a.Cin_g + ci0 + c] : 0.f;
        }
        for (int i = tid; i < CV_C * CK; i += 256) {
            const int co = i / CK, r = i - co * CK, c = r / a.k;
            Ws[r * CV_CP + co] = (c0 + co < a.Cout_g && c < nci) ? a.w[((size_t)(g * a.Cout_g + c0 + co) * a.Cin_g + ci0) * a.k + r] : 0.f;
        }
        __syncthreads();
        float part[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) part[i][j] = 0.f;
        for (int c = 0; c < nci; ++c) {
            for (int kk = 0; kk < a.k; ++kk) {
                const float* wr = Ws + (c * a.k + kk) * CV_CP + tx;
                const float* xr = Xs + (ty * a.s + kk) * CIp + c;
                float wv[4], xv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) wv[j] = wr[16 * j];
#pragma unroll
                for (int i = 0; i < 4; ++i) xv[i] = xr[16 * i * a.s * CIp];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) part[i][j] = fmaf(xv[i], wv[j], part[i][j]);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] += part[i][j];
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long t = t0 + ty + 16 * i;
        if (t >= a.Tout) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int co = c0 + tx + 16 * j;
            if (co >= a.Cout_g) continue;
            const int ch = g * a.Cout_g + co;
            float v = acc[i][j];
            if (a.bias) v += a.bias[ch];
            if (a.gelu) v = gelu_erf_f(v);
            if (a.res) v += a.res[(size_t)t * a.ldres + ch];
            a.y[(size_t)t * a.ldy + ch] = v;
        }
    }
}

svi_status launch_conv1d(W2vConv a, hipStream_t st) {
    a.CI = std::max(1, std::min(std::min(16, 128 / a.k), a.Cin_g));
    const int rows = (CV_T - 1) * a.s + a.k;
    const size_t lds = ((size_t)rows * (a.CI + 1) + (size_t)a.CI * a.k * CV_CP) * 4;
    SVI_REQUIRE(lds <= 64 * 1024, "audio encoder convolution: kernel %d, stride %d need %zu B of LDS (limit 65536)", a.k, a.s, lds);
    const long tiles = (a.Tout + CV_T - 1) / CV_T;
    const long ct = (long)a.groups * ((a.Cout_g + CV_C - 1) / CV_C);
    SVI_REQUIRE(tiles > 0 && tiles < 0x7fffffffL && ct > 0 && ct <= 65535, "audio encoder convolution: launch grid out of range");
    hipLaunchKernelGGL(w2v_conv1d_kernel, dim3((unsigned)tiles, (unsigned)ct), dim3(256), lds, st, a);
    SVI_LAUNCH_CHECK();
    return SVI_OK;
}

// ---------------------------------------------------------------- statistics over time --------------------------------------------
// x [T, C]: per channel the mean and the biased variance over all T rows (the waveform: C = 1; GroupNorm(C, C) of the first layer: one group per
// channel).  Two passes — the sum, then the sum of squared distances from the mean — each as fp32 partial sums over chunks of ST_CHUNK rows that one
// thread per channel adds up in double.
constexpr int ST_CHUNK = 1024;
__global__ __launch_bounds__(256) void w2v_colsum_kernel(const float* __restrict__ x, long T, int C, int ld, const float* __restrict__ mean,
                                                         float* __restrict__ part) {
    __shared__ float sh[4][64];
    const int lane = threadIdx.x & 63, rl = threadIdx.x >> 6, c = blockIdx.y * 64 + lane;
    const long r0 = (long)blockIdx.x * ST_CHUNK, r1 = min(r0 + (long)ST_CHUNK, T);
    float s = 0.f;
    if (c < C) {
        const float m = mean ? mean[c] : 0.f;
        for (long r = r0 + rl; r < r1; r += 4) {
            const float d = x[(size_t)r * ld + c] - m;
            s += mean ? d * d : d;
        }
    }
    sh[rl][lane] = s;
    __syncthreads();
    if (rl == 0 && c < C) part[(size_t)blockIdx.x * C + c] = (sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane]);
}
__global__ void w2v_colstat_kernel(const float* __restrict__ part, int chunks, int C, long T, float* __restrict__ stat) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (int i = 0; i < chunks; ++i) s += (double)part[(size_t)i * C + c];
    stat[c] = (float)(s / (double)T);
}
// y = (x - mean) / sqrt(var + eps) [* w + b] [GELU]; y may be x
__global__ void w2v_colnorm_kernel(const float* x, float* y, long n, int C, const float* __restrict__ mean,
                                   const float* __restrict__ var, float eps, const float* __restrict__ w, const float* __restrict__ b, int gelu) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    float v = (x[i] - mean[c]) / sqrtf(var[c] + eps);
    if (w) v = v * w[c] + b[c];
    if (gelu) v = gelu_erf_f(v);
    y[i] = v;
}

// ---------------------------------------------------------------- interpolation, output --------------------------------------------
// F.interpolate(mode='linear', align_corners=True) along time: source position = i (Tin - 1) / (Tout - 1) in fp32 (0 when Tout == 1)
__global__ void w2v_interp_kernel(const float* __restrict__ x, long Tin, float* __restrict__ y, int Tout, int C, float scale) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)Tout * C) return;
    const int t = (int)(i / C), c = (int)(i - (long)t * C);
    const float pos = scale * (float)t;
    long i0 = (long)pos;
    if (i0 > Tin - 1) i0 = Tin - 1;
    const long i1 = i0 + (i0 < Tin - 1 ? 1 : 0);
    const float l1 = pos - (float)i0, l0 = 1.0f - l1;
    y[i] = l0 * x[(size_t)i0 * C + c] + l1 * x[(size_t)i1 * C + c];
}

// rows of one block's output -> out[t][layer][:]
template <typename T>
__global__ void w2v_write_layer_kernel(const float* __restrict__ x, T* __restrict__ out, int rows, int dim, int layer, int layers) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)rows * dim) return;
    const int t = (int)(i / dim), c = (int)(i - (long)t * dim);
    out[((size_t)t * layers + layer) * dim + c] = (T)x[i];
}

}  // namespace

struct svi_w2v : EncHandle {
    svi_w2v_config cfg{};
    int max_frames = W2V_MAX_FRAMES;                 // svi_w2v_set_max_frames
};

namespace {

const char* const W2V_CONV = "feature_extractor.conv_layers.";
// Wav2Vec2Model's state dict with the positional convolution's weight norm folded (svi_hip.encoders.fold_weight_norm)
void w2v_table(const svi_w2v_config& c, EncTable* t) {
    const int64_t C = c.conv_dim, H = c.hidden, F = c.ffn;
    t->noun = "audio encoder"; t->bind_fn = "svi_w2v_bind_weight"; t->max_rank = 3;
    t->dtype = SVI_F32; t->dtype_words = "fp32 (the reference runs this model in fp32)";
    t->layer_prefix = "encoder.layers."; t->layers = t->layers_used = c.num_layers;
    for (int i = 0; i < W2V_CONVS; ++i) t->rows.push_back({W2V_CONV + std::to_string(i) + ".conv.weight", {C, i == 0 ? 1 : C, W2V_KERNEL[i]}, 0});
    const EncRow rest[] = {{std::string(W2V_CONV) + "0.layer_norm.weight", {C}, 0}, {std::string(W2V_CONV) + "0.layer_norm.bias", {C}, 0},
                           {"feature_projection.layer_norm.weight", {C}, 0}, {"feature_projection.layer_norm.bias", {C}, 0},
                           {"feature_projection.projection.weight", {H, C}, 0}, {"feature_projection.projection.bias", {H}, 0},
                           {"encoder.pos_conv_embed.conv.weight", {H, H / c.pos_groups, c.pos_kernel}, 0}, {"encoder.pos_conv_embed.conv.bias", {H}, 0},
                           {"encoder.layer_norm.weight", {H}, 0}, {"encoder.layer_norm.bias", {H}, 0},
                           {"masked_spec_embed", {}, ENC_UNUSED},                       // training-time masking only
                           {"attention.q_proj.weight", {H, H}, ENC_LAYER}, {"attention.q_proj.bias", {H}, ENC_LAYER},
                           {"attention.k_proj.weight", {H, H}, ENC_LAYER}, {"attention.k_proj.bias", {H}, ENC_LAYER},
                           {"attention.v_proj.weight", {H, H}, ENC_LAYER}, {"attention.v_proj.bias", {H}, ENC_LAYER},
                           {"attention.out_proj.weight", {H, H}, ENC_LAYER}, {"attention.out_proj.bias", {H}, ENC_LAYER},
                           {"layer_norm.weight", {H}, ENC_LAYER}, {"layer_norm.bias", {H}, ENC_LAYER},
                           {"feed_forward.intermediate_dense.weight", {F, H}, ENC_LAYER}, {"feed_forward.intermediate_dense.bias", {F}, ENC_LAYER},
                           {"feed_forward.output_dense.weight", {H, F}, ENC_LAYER}, {"feed_forward.output_dense.bias", {H}, ENC_LAYER},
                           {"final_layer_norm.weight", {H}, ENC_LAYER}, {"final_layer_norm.bias", {H}, ENC_LAYER}};
    t->rows.insert(t->rows.end(), std::begin(rest), std::end(rest));
}

// what both entry points refuse before anything touches the device
svi_status w2v_check_request(svi_w2v* h, const void* samples, int64_t n_samples, int32_t seq_len, const char* who) {
    SVI_REQUIRE(h && samples, "%s: null argument", who);
    SVI_REQUIRE(n_samples >= 1, "%s: %lld samples (need at least 1)", who, (long long)n_samples);
    SVI_REQUIRE(seq_len >= 1, "%s: seq_len %d (need at least 1: 1/25 s of audio)", who, seq_len);
    if (h->max_frames == W2V_MAX_FRAMES)
        SVI_REQUIRE(seq_len <= W2V_MAX_FRAMES,
                    "%s: seq_len %d is above the encoder attention's limit of 2048 keys (about 81 s of audio at 25 frames per second); "
                    "encode the audio in pieces, or raise this handle's limit with svi_w2v_set_max_frames (up to %d)", who, seq_len, W2V_FRAME_CAP);
    SVI_REQUIRE(seq_len <= h->max_frames, "%s: seq_len %d is above this handle's limit of %d frames (svi_w2v_set_max_frames, up to %d)", who, seq_len,
                h->max_frames, W2V_FRAME_CAP);
    SVI_REQUIRE(n_samples <= 0x7fffffffLL, "%s: %lld samples (limit 2^31 - 1)", who, (long long)n_samples);
    SVI_REQUIRE(w2v_frames_after((long)n_samples, W2V_CONVS) >= 1, "%s: %lld samples are shorter than the convolution stack's receptive field (400 samples)",
                who, (long long)n_samples);
    // the largest launches with one thread per value: the first layer's GroupNorm over [frames_1, conv_dim], the feed-forward's GELU over [seq_len, ffn]
    const long t1 = w2v_frames_after((long)n_samples, 1), wide = std::max(std::max(h->cfg.conv_dim, h->cfg.hidden), h->cfg.ffn);
    SVI_REQUIRE(t1 * h->cfg.conv_dim <= W2V_LAUNCH_ELEMS, "%s: %lld samples are %ld rows of %d channels after the first convolution layer (limit 2^32 - 256 values)",
                who, (long long)n_samples, t1, h->cfg.conv_dim);
    SVI_REQUIRE((long)seq_len * wide <= W2V_LAUNCH_ELEMS, "%s: seq_len %d of %ld channels (limit 2^32 - 256 values)", who, seq_len, wide);
    SVI_TRY(svi_w2v_check_bound(h));
    return SVI_OK;
}

// Stages of the forward, in order (svi_w2v_forward_stage): the tensor a stage names is copied out and the forward ends there.
enum { ST_WAVE = 0, ST_CONV0 = 1, ST_INTERP = 8, ST_PROJ = 9, ST_POS = 10, ST_ENC_LN = 11, ST_LAYER0 = 12, ST_ALL = 1 << 20 };

svi_status w2v_run(svi_w2v* h, const float* samples, long n, int S, int stage, float* stage_out, int64_t capacity, void* out, svi_dtype out_dtype,
                   hipStream_t st) {
    const svi_w2v_config& c = h->cfg;
    const int C = c.conv_dim, H = c.hidden, F = c.ffn, D = H / c.num_heads;
    long T[W2V_CONVS + 1];
    for (int i = 0; i <= W2V_CONVS; ++i) T[i] = w2v_frames_after(n, i);
    const long Tf = T[W2V_CONVS];
    W2vBufs bufs;
    SVI_TRY(svi_enc_carve(h, [&](EncArena& a) { bufs = w2v_buffers(a, n, T[1], T[2], ST_CHUNK, S, C, H, F); }));
    float *const Wv = bufs.Wv, *const A = bufs.A, *const B = bufs.B, *const Part = bufs.Part, *const Stat = bufs.Stat, *const I0 = bufs.I0, *const I1 = bufs.I1,
          *const X = bufs.X, *const Y = bufs.Y, *const N1 = bufs.N1, *const At = bufs.At, *const Big = bufs.Big;       // (not a structured binding: lambdas below capture them)
#define W(k) SVI_ENC_W(float, h->w, k)
    // the tensor a stage names -> the caller's buffer; true: the forward ends here
    auto tap = [&](int which, const float* src, size_t count, bool* done) -> svi_status {
        *done = false;
        if (stage != which) return SVI_OK;
        SVI_REQUIRE((int64_t)count <= capacity, "svi_w2v_forward_stage: stage %d holds %zu values, the buffer %lld", which, count, (long long)capacity);
        SVI_CHECK_HIP(hipMemcpyAsync(stage_out, src, count * 4, hipMemcpyDeviceToDevice, st));
        *done = true;
        return SVI_OK;
    };
    // mean and biased variance over the rows of x [rows, cols] -> Stat[0 .. cols), Stat[cols .. 2 cols)
    auto stats = [&](const float* x, long rows, int cols) -> svi_status {
        const int chunks = (int)((rows + ST_CHUNK - 1) / ST_CHUNK);
        const dim3 grid((unsigned)chunks, (unsigned)((cols + 63) / 64));
        hipLaunchKernelGGL(w2v_colsum_kernel, grid, dim3(256), 0, st, x, rows, cols, cols, (const float*)nullptr, Part);
        hipLaunchKernelGGL(w2v_colstat_kernel, dim3((cols + 63) / 64), dim3(64), 0, st, Part, chunks, cols, rows, Stat);
        hipLaunchKernelGGL(w2v_colsum_kernel, grid, dim3(256), 0, st, x, rows, cols, cols, (const float*)Stat, Part);
        hipLaunchKernelGGL(w2v_colstat_kernel, dim3((cols + 63) / 64), dim3(64), 0, st, Part, chunks, cols, rows, Stat + cols);
        SVI_LAUNCH_CHECK();
        return SVI_OK;
    };
    bool done = false;
    // ---- waveform normalisation
    SVI_TRY(stats(samples, n, 1));
    hipLaunchKernelGGL(w2v_colnorm_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, samples, Wv, n, 1, Stat, Stat + 1, W2V_WAVE_EPS,
                       (const float*)nullptr, (const float*)nullptr, 0);
    SVI_LAUNCH_CHECK();
    SVI_TRY(tap(ST_WAVE, Wv, (size_t)n, &done));
    if (done) return SVI_OK;
    // ---- feature extractor
    const float* cur = Wv;
    for (int i = 0; i < W2V_CONVS; ++i) {
        float* dst = (i % 2 == 0) ? A : B;
        W2vConv a{};
        a.x = cur; a.Tin = T[i]; a.ldx = i == 0 ? 1 : C;
        a.w = W(W2V_CONV + std::to_string(i) + ".conv.weight");
        a.y = dst; a.ldy = C; a.Tout = T[i + 1];
        a.Cin_g = i == 0 ? 1 : C; a.Cout_g = C; a.groups = 1; a.k = W2V_KERNEL[i]; a.s = W2V_STRIDE[i]; a.pad = 0;
        a.gelu = i == 0 ? 0 : 1;                                      // layer 0: GroupNorm comes between the convolution and the GELU
        SVI_TRY(launch_conv1d(a, st));
        if (i == 0) {
            SVI_TRY(stats(dst, T[1], C));
            const long cnt = T[1] * C;
            hipLaunchKernelGGL(w2v_colnorm_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, (const float*)dst, dst, cnt, C, Stat, Stat + C,
                               W2V_GROUPNORM_EPS, W(std::string(W2V_CONV) + "0.layer_norm.weight"), W(std::string(W2V_CONV) + "0.layer_norm.bias"), 1);
            SVI_LAUNCH_CHECK();
        }
        SVI_TRY(tap(ST_CONV0 + i, dst, (size_t)T[i + 1] * C, &done));
        if (done) return SVI_OK;
        cur = dst;
    }
    // ---- interpolation to seq_len, feature projection
    {
        const float scale = S > 1 ? (float)(Tf - 1) / (float)(S - 1) : 0.f;
        const long cnt = (long)S * C;
        hipLaunchKernelGGL(w2v_interp_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, cur, Tf, I0, S, C, scale);
        SVI_LAUNCH_CHECK();
    }
    SVI_TRY(tap(ST_INTERP, I0, (size_t)S * C, &done));
    if (done) return SVI_OK;
    SVI_TRY(svi_launch_layernorm_f32(I0, I1, W("feature_projection.layer_norm.weight"), W("feature_projection.layer_norm.bias"), S, C, c.eps, st));
    SVI_TRY(svi_launch_gemm_f32(I1, C, W("feature_projection.projection.weight"), C, W("feature_projection.projection.bias"), Y, H, S, H, C, nullptr, 0, st));
    SVI_TRY(tap(ST_PROJ, Y, (size_t)S * H, &done));
    if (done) return SVI_OK;
    // ---- positional convolution: padding k/2 on both sides, the last output of an even kernel dropped -> frame t reads rows t - k/2 .. t - k/2 + k - 1
    {
        W2vConv a{};
        a.x = Y; a.Tin = S; a.ldx = H;
        a.w = W("encoder.pos_conv_embed.conv.weight"); a.bias = W("encoder.pos_conv_embed.conv.bias");
        a.res = stage == ST_POS ? nullptr : Y; a.ldres = H;          // the stage is the module's own output; the forward adds its input
        a.y = N1; a.ldy = H; a.Tout = S;
        a.Cin_g = H / c.pos_groups; a.Cout_g = H / c.pos_groups; a.groups = c.pos_groups; a.k = c.pos_kernel; a.s = 1; a.pad = c.pos_kernel / 2;
        a.gelu = 1;
        SVI_TRY(launch_conv1d(a, st));
    }
    SVI_TRY(tap(ST_POS, N1, (size_t)S * H, &done));
    if (done) return SVI_OK;
    SVI_TRY(svi_launch_layernorm_f32(N1, X, W("encoder.layer_norm.weight"), W("encoder.layer_norm.bias"), S, H, c.eps, st));
    SVI_TRY(tap(ST_ENC_LN, X, (size_t)S * H, &done));
    if (done) return SVI_OK;
    // ---- post-norm blocks
    const float scale = 1.0f / sqrtf((float)D);
    for (int i = 0; i < c.num_layers; ++i) {
        const std::string b = "encoder.layers." + std::to_string(i) + ".";
        float* QKV = Big;
        SVI_TRY(svi_launch_gemm_f32(X, H, W(b + "attention.q_proj.weight"), H, W(b + "attention.q_proj.bias"), QKV, 3 * H, S, H, H, nullptr, 0, st));
        SVI_TRY(svi_launch_gemm_f32(X, H, W(b + "attention.k_proj.weight"), H, W(b + "attention.k_proj.bias"), QKV + H, 3 * H, S, H, H, nullptr, 0, st));
        SVI_TRY(svi_launch_gemm_f32(X, H, W(b + "attention.v_proj.weight"), H, W(b + "attention.v_proj.bias"), QKV + 2 * H, 3 * H, S, H, H, nullptr, 0, st));
        SVI_TRY(svi_launch_enc_attention_f32(QKV, 3 * H, QKV + H, 3 * H, QKV + 2 * H, 3 * H, At, H, S, S, c.num_heads, D, scale, SVI_ENC_ATT_AUTO, st));
        SVI_TRY(svi_launch_gemm_f32(At, H, W(b + "attention.out_proj.weight"), H, W(b + "attention.out_proj.bias"), Y, H, S, H, H, X, H, st));
        SVI_TRY(svi_launch_layernorm_f32(Y, N1, W(b + "layer_norm.weight"), W(b + "layer_norm.bias"), S, H, c.eps, st));
        SVI_TRY(svi_launch_gemm_f32(N1, H, W(b + "feed_forward.intermediate_dense.weight"), H, W(b + "feed_forward.intermediate_dense.bias"), Big, F, S, F, H,
                                    nullptr, 0, st));
        SVI_TRY(svi_launch_gelu_erf_f32(Big, (long)S * F, st));
        SVI_TRY(svi_launch_gemm_f32(Big, F, W(b + "feed_forward.output_dense.weight"), F, W(b + "feed_forward.output_dense.bias"), Y, H, S, H, F, N1, H, st));
        SVI_TRY(svi_launch_layernorm_f32(Y, X, W(b + "final_layer_norm.weight"), W(b + "final_layer_norm.bias"), S, H, c.eps, st));
        SVI_TRY(tap(ST_LAYER0 + i, X, (size_t)S * H, &done));
        if (done) return SVI_OK;
        if (out) {
            const long cnt = (long)S * H;
            const dim3 grid((unsigned)((cnt + 255) / 256));
            if (out_dtype == SVI_F32)
                hipLaunchKernelGGL(w2v_write_layer_kernel<float>, grid, dim3(256), 0, st, (const float*)X, reinterpret_cast<float*>(out), S, H, i, c.num_layers);
            else
                hipLaunchKernelGGL(w2v_write_layer_kernel<bf16>, grid, dim3(256), 0, st, (const float*)X, reinterpret_cast<bf16*>(out), S, H, i, c.num_layers);
            SVI_LAUNCH_CHECK();
        }
    }
    SVI_REQUIRE(stage == ST_ALL, "svi_w2v_forward_stage: no stage %d (0 .. %d)", stage, ST_LAYER0 + c.num_layers - 1);
    return SVI_OK;
#undef W
}

}  // namespace

extern "C" svi_status svi_w2v_create(const svi_w2v_config* cfg, svi_w2v** out) {
    SVI_REQUIRE(cfg && out, "svi_w2v_create: null argument");
    SVI_REQUIRE(cfg->conv_dim > 0 && cfg->conv_dim % 4 == 0 && cfg->hidden > 0 && cfg->hidden % 4 == 0 && cfg->ffn > 0 && cfg->ffn % 4 == 0 &&
                cfg->num_heads > 0 && cfg->hidden % cfg->num_heads == 0 && cfg->num_layers > 0 && cfg->eps > 0.f,
                "svi_w2v_create: conv_dim, hidden and ffn must be positive multiples of 4, heads must divide hidden, layers and eps positive");
    SVI_REQUIRE(cfg->pos_kernel >= 1 && cfg->pos_kernel <= 128 && cfg->pos_groups >= 1 && cfg->hidden % cfg->pos_groups == 0,
                "svi_w2v_create: positional convolution kernel %d (1..128) with %d groups over %d channels", cfg->pos_kernel, cfg->pos_groups, cfg->hidden);
    const int D = cfg->hidden / cfg->num_heads;
    SVI_REQUIRE(svi_enc_head_dim_ok(D), "svi_w2v_create: head dim %d (the encoder attention has 32, 64, 80, 128)", D);
    svi_w2v* h = new (std::nothrow) svi_w2v();
    if (!h) { svi_set_error("out of host memory"); return SVI_ERR_OOM; }
    h->cfg = *cfg;
    w2v_table(*cfg, &h->w);
    *out = h;
    return SVI_OK;
}

extern "C" svi_status svi_w2v_destroy(svi_w2v* h) {
    if (!h) return SVI_OK;
    if (h->ws) (void)hipFree(h->ws);
    delete h;
    return SVI_OK;
}

extern "C" svi_status svi_w2v_bind_weight(svi_w2v* h, const char* name, const void* dev_ptr, svi_dtype dtype, const int64_t* shape, int32_t rank) {
    SVI_REQUIRE(h, "svi_w2v_bind_weight: bad argument");
    return h->w.bind(name, dev_ptr, dtype, shape, rank);
}

extern "C" svi_status svi_w2v_check_bound(svi_w2v* h) {
    SVI_REQUIRE(h, "null handle");
    return h->w.check_bound();
}

extern "C" svi_status svi_w2v_set_max_frames(svi_w2v* h, int32_t max_frames) {
    SVI_REQUIRE(h, "svi_w2v_set_max_frames: null handle");
    SVI_REQUIRE(max_frames >= 1 && max_frames <= W2V_FRAME_CAP, "svi_w2v_set_max_frames: max_frames %d (1 .. %d)", max_frames, W2V_FRAME_CAP);
    h->max_frames = max_frames;
    return SVI_OK;
}

extern "C" svi_status svi_w2v_frames(int64_t n_samples, int64_t* out) {
    SVI_REQUIRE(out, "svi_w2v_frames: null argument");
    SVI_REQUIRE(n_samples >= 0 && n_samples <= 0x7fffffffLL, "svi_w2v_frames: %lld samples (0 .. 2^31 - 1)", (long long)n_samples);
    *out = w2v_frames_after((long)n_samples, W2V_CONVS);
    return SVI_OK;
}

extern "C" svi_status svi_w2v_forward(svi_w2v* h, const float* samples, int64_t n_samples, int32_t seq_len, void* out, svi_dtype out_dtype,
                                      svi_stream stream) {
    SVI_REQUIRE(out, "svi_w2v_forward: null argument");
    SVI_REQUIRE(out_dtype == SVI_F32 || out_dtype == SVI_BF16, "svi_w2v_forward: the output is fp32 or bf16");
    SVI_TRY(w2v_check_request(h, samples, n_samples, seq_len, "svi_w2v_forward"));
    SVI_REQUIRE_DEVICE(h);
    return w2v_run(h, samples, (long)n_samples, seq_len, ST_ALL, nullptr, 0, out, out_dtype, reinterpret_cast<hipStream_t>(stream));
}

extern "C" svi_status svi_w2v_forward_stage(svi_w2v* h, const float* samples, int64_t n_samples, int32_t seq_len, int32_t stage, float* out,
                                            int64_t capacity, svi_stream stream) {
    SVI_REQUIRE(out && capacity > 0, "svi_w2v_forward_stage: null argument");
    SVI_TRY(w2v_check_request(h, samples, n_samples, seq_len, "svi_w2v_forward_stage"));
    SVI_REQUIRE(stage >= 0 && stage < ST_LAYER0 + h->cfg.num_layers, "svi_w2v_forward_stage: no stage %d (0 .. %d)", stage, ST_LAYER0 + h->cfg.num_layers - 1);
    SVI_REQUIRE_DEVICE(h);
    return w2v_run(h, samples, (long)n_samples, seq_len, stage, out, capacity, nullptr, SVI_F32, reinterpret_cast<hipStream_t>(stream));
}
