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
// Activations are time-major [T, C].  The projections run on the exact-fp32 MFMA GEMM, attention and LayerNorm on the fp32 kernels of the image
// encoder (svi_encoders.hip).  New here: one direct convolution kernel (a window of k rows of a time-major activation is k * Cin contiguous floats;
// it serves the feature extractor's layers and, with groups and a symmetric pad, the positional convolution), the statistics over time of the
// waveform and of the first layer's GroupNorm, the interpolation, and the writer of the [seq_len, layers, hidden] output.
//
// Compiled as ONE translation unit with svi_encoders.hip (included below; svi_hip/build.py lists this file in its place): the fp32 attention, LayerNorm
// and GELU kernels this encoder launches are that file's, in its unnamed namespace, and stay there untouched — the same kernels, the same bits.
//
// Length: the reference hands the whole file to the model in one call (every frame attends to every other, the waveform statistics are the file's), so
// a file cannot be encoded in pieces.  A handle serves up to max_frames frames per call: 2048 when it is made (the resident attention kernel's key
// count, about 81 s), up to W2V_FRAME_CAP = 65536 (43.7 min) after svi_w2v_set_max_frames.  Up to 2048 frames the attention is the resident kernel,
// above it the streaming kernel below (online softmax, fp32 throughout, LDS independent of the key count); nothing else in the forward
// depends on the length.  svi_encoder_attention_f32 is that attention alone, as an operator.
#include "svi_encoders.hip"

namespace {

constexpr int W2V_CONVS = 7;
const int W2V_KERNEL[W2V_CONVS] = {10, 3, 3, 3, 3, 2, 2};
const int W2V_STRIDE[W2V_CONVS] = {5, 2, 2, 2, 2, 2, 2};
constexpr int W2V_MAX_FRAMES = 2048;              // a fresh handle's frame limit: the resident encoder attention's key limit (svi_encoders.hip)
constexpr int W2V_FRAME_CAP = 65536;              // the most svi_w2v_set_max_frames grants (43.7 min at 25 frames per second); the audit is in DESIGN §4
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

// ---------------------------------------------------------------- streaming attention ----------------------------------------------
// The encoder attention of svi_encoders.hip (enc_attention_kernel, ENC_RQ query rows per workgroup) for ANY key count, plain fp32 only — the audio
// encoder past 2048 frames.  It lives here and not beside the resident kernel because that file is also the T5 / CLIP encoders' and stays byte for
// byte what the committed profiles were collected on.  The key axis is walked in tiles of ENC_KT keys and a
// query row keeps a running maximum m, a running sum l and an accumulator that is rescaled when the maximum moves (online softmax), so LDS and
// registers do not grow with Lk.  One workgroup = one head x ENC_RQ query rows, as there.  Per tile:
//   scores   thread <-> key: 16 dot products against the staged query rows; keys past Lk score -inf
//   softmax  wave w owns rows 4w..4w+3: m' = max(m, tile max) (finite unless the caller's scores are -inf: a tile holds at least one key);
//            alpha = exp(m - m'), 0 while m is still -inf (no (-inf) - (-inf)); p = exp(s - m'); l = l alpha + sum p
//   P.V      thread <-> (row group, channel) as there: acc = acc alpha + sum_j p_j v_j, the tile's sum formed on its own in four interleaved chains
// and O = acc / l after the last tile.  Every value is fp32; a term exp(s - m') that underflows is an exact zero and leaves acc and l as they were.
// LDS: (16 D + 16 (ENC_KT + 1) + 48) x 4 B = 24.8 KiB at D = 128; registers: 16 score sums or 4 x RPG (<= 32) partial sums per thread.
#define ENC_KT 256
constexpr int ENC_KTP = ENC_KT + 1;               // row stride of the tile's scores: rows of two row groups in one wave fall on different banks
template <int D>
__global__ __launch_bounds__(256) void enc_attention_stream_kernel(const float* __restrict__ Q, int ldq, const float* __restrict__ K, int ldk,
                                                                   const float* __restrict__ V, int ldv, float* __restrict__ O, int ldo, int Lq, int Lk,
                                                                   float scale) {
    __shared__ __attribute__((aligned(16))) float Qs[ENC_RQ * D];
    __shared__ float S[ENC_RQ * ENC_KTP];
    __shared__ float alpha_s[ENC_RQ], l_s[ENC_RQ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, head = blockIdx.y, q0 = blockIdx.x * ENC_RQ;
    const int nq = min(ENC_RQ, Lq - q0);
    for (int i = tid; i < ENC_RQ * D; i += 256) {
        const int r = i / D, c = i - r * D;
        Qs[i] = r < nq ? Q[(size_t)(q0 + r) * ldq + head * D + c] : 0.f;
    }
    float m_run[4], l_run[4];                     // of rows 4 wave .. 4 wave + 3, the same in every lane of the wave
#pragma unroll
    for (int i = 0; i < 4; ++i) { m_run[i] = -INFINITY; l_run[i] = 0.f; }
    constexpr int NG = 256 / D, RPG = (ENC_RQ + NG - 1) / NG;
    const int g = tid / D, c = tid - g * D;
    float acc[RPG];
#pragma unroll
    for (int r = 0; r < RPG; ++r) acc[r] = 0.f;
    __syncthreads();
    for (int k0 = 0; k0 < Lk; k0 += ENC_KT) {
        const int nk = min(ENC_KT, Lk - k0);
        // ---- scores of this tile: thread <-> key
        {
            float s[ENC_RQ];
#pragma unroll
            for (int r = 0; r < ENC_RQ; ++r) s[r] = 0.f;
            if (tid < nk) {
                const float* kp = K + (size_t)(k0 + tid) * ldk + head * D;
#pragma unroll 4
                for (int cc = 0; cc < D; cc += 4) {
                    float kv[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) kv[e] = kp[cc + e];
#pragma unroll
                    for (int r = 0; r < ENC_RQ; ++r) {
                        const f32x4 qv = *reinterpret_cast<const f32x4*>(Qs + r * D + cc);
                        s[r] = fmaf(qv[0], kv[0], s[r]); s[r] = fmaf(qv[1], kv[1], s[r]);
                        s[r] = fmaf(qv[2], kv[2], s[r]); s[r] = fmaf(qv[3], kv[3], s[r]);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < ENC_RQ; ++r) S[r * ENC_KTP + tid] = tid < nk ? s[r] * scale : -INFINITY;
        }
        __syncthreads();
        // ---- running maximum and sum; the tile's scores become its unnormalised probabilities
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float* row = S + (4 * wave + i) * ENC_KTP;
            float sv[ENC_KT / 64];
            float mt = -INFINITY;
#pragma unroll
            for (int j = 0; j < ENC_KT / 64; ++j) { sv[j] = row[lane + 64 * j]; mt = fmaxf(mt, sv[j]); }
            const float m_new = fmaxf(m_run[i], wave_max(mt));
            const float alpha = m_run[i] == -INFINITY ? 0.f : expf(m_run[i] - m_new);
            const float m_sub = m_new == -INFINITY ? 0.f : m_new;          // every score so far is -inf (the caller's own): the tile's terms are zeros
            float sum = 0.f;
#pragma unroll
            for (int j = 0; j < ENC_KT / 64; ++j) { const float e = expf(sv[j] - m_sub); row[lane + 64 * j] = e; sum += e; }
            l_run[i] = l_run[i] * alpha + wave_sum(sum);
            m_run[i] = m_new;
            if (lane == 0) alpha_s[4 * wave + i] = alpha;
        }
        __syncthreads();
        // ---- acc = acc alpha + P V of this tile
        if (g < NG) {
            float part[RPG][4];
#pragma unroll
            for (int r = 0; r < RPG; ++r)
#pragma unroll
                for (int e = 0; e < 4; ++e) part[r][e] = 0.f;
            const float* vp = V + (size_t)k0 * ldv + head * D + c;
            int j = 0;
            for (; j + 3 < nk; j += 4) {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = vp[(size_t)(j + e) * ldv];
#pragma unroll
                for (int r = 0; r < RPG; ++r) {
                    const int row = g * RPG + r;
                    if (row < ENC_RQ) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) part[r][e] = fmaf(S[row * ENC_KTP + j + e], v[e], part[r][e]);
                    }
                }
            }
            for (; j < nk; ++j) {
                const float v = vp[(size_t)j * ldv];
#pragma unroll
                for (int r = 0; r < RPG; ++r) {
                    const int row = g * RPG + r;
                    if (row < ENC_RQ) part[r][0] = fmaf(S[row * ENC_KTP + j], v, part[r][0]);
                }
            }
#pragma unroll
            for (int r = 0; r < RPG; ++r) {
                const int row = g * RPG + r;
                if (row < ENC_RQ) acc[r] = acc[r] * alpha_s[row] + ((part[r][0] + part[r][1]) + (part[r][2] + part[r][3]));
            }
        }
        __syncthreads();
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) l_s[4 * wave + i] = l_run[i];
    }
    __syncthreads();
    if (g < NG) {
#pragma unroll
        for (int r = 0; r < RPG; ++r) {
            const int row = g * RPG + r;
            if (row < nq) O[(size_t)(q0 + row) * ldo + head * D + c] = acc[r] / l_s[row];
        }
    }
}

svi_status launch_enc_attention_stream(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo, int Lq, int Lk,
                                       int heads, int D, float scale, hipStream_t st) {
    SVI_REQUIRE(Lq > 0 && Lk > 0 && heads > 0 && heads <= 65535, "streaming encoder attention: %d queries, %d keys, %d heads", Lq, Lk, heads);
    dim3 grid((Lq + ENC_RQ - 1) / ENC_RQ, heads), block(256);
#define ENC_CASE(DD)                                                                                                                        \
    case DD:                                                                                                                                \
        hipLaunchKernelGGL((enc_attention_stream_kernel<DD>), grid, block, 0, st, Q, ldq, K, ldk, V, ldv, O, ldo, Lq, Lk, scale);             \
        break;
    switch (D) {
        ENC_CASE(32) ENC_CASE(64) ENC_CASE(80) ENC_CASE(128)
        default: svi_set_error("streaming encoder attention: head dim %d (supported: 32, 64, 80, 128)", D); return SVI_ERR_UNSUPPORTED;
    }
#undef ENC_CASE
    SVI_LAUNCH_CHECK();
    return SVI_OK;
}

// the fp32 pieces of svi_encoders.hip, by the names this file calls them.  Attention: the resident kernel (whole score rows in LDS) up to its 2048
// keys — the same launch and the same bits as before there was a choice — and the streaming kernel above.
svi_status svi_launch_enc_attention_f32(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo, int Lq, int Lk,
                                        int heads, int D, float scale, hipStream_t st) {
    if (Lk > W2V_MAX_FRAMES) return launch_enc_attention_stream(Q, ldq, K, ldk, V, ldv, O, ldo, Lq, Lk, heads, D, scale, st);
    return launch_enc_attention<float, false>(Q, ldq, K, ldk, V, ldv, O, ldo, Lq, Lk, heads, D, scale, nullptr, nullptr, 0, st);
}
svi_status svi_launch_layernorm_f32(const float* x, float* out, const float* w, const float* b, int rows, int dim, float eps, hipStream_t st) {
    hipLaunchKernelGGL(layernorm_f32_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, x, out, w, b, rows, dim, eps);
    SVI_LAUNCH_CHECK();
    return SVI_OK;
}
svi_status svi_launch_gelu_erf_f32(float* x, long n, hipStream_t st) {
    hipLaunchKernelGGL(gelu_erf_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, n);
    SVI_LAUNCH_CHECK();
    return SVI_OK;
}

}  // namespace

struct svi_w2v {
    int device = -1;
    svi_w2v_config cfg{};
    std::map<std::string, Param> w;
    char* ws = nullptr; size_t ws_bytes = 0;
    int max_frames = W2V_MAX_FRAMES;                 // svi_w2v_set_max_frames
};

namespace {

bool w2v_expected(const svi_w2v_config& c, const std::string& name, std::vector<int64_t>* shape, bool* used) {
    const int64_t C = c.conv_dim, H = c.hidden, F = c.ffn;
    *used = true;
    if (name == "masked_spec_embed") { *used = false; shape->clear(); return true; }             // training-time masking only
    if (name.rfind("feature_extractor.conv_layers.", 0) == 0) {
        char* end = nullptr;
        const char* s = name.c_str() + 30;
        const long i = strtol(s, &end, 10);
        if (end == s || *end != '.' || i < 0 || i >= W2V_CONVS) return false;
        const std::string rest(end + 1);
        if (rest == "conv.weight") { *shape = {C, i == 0 ? 1 : C, W2V_KERNEL[i]}; return true; }
        if (i == 0 && (rest == "layer_norm.weight" || rest == "layer_norm.bias")) { *shape = {C}; return true; }
        return false;
    }
    if (name == "feature_projection.layer_norm.weight" || name == "feature_projection.layer_norm.bias") { *shape = {C}; return true; }
    if (name == "feature_projection.projection.weight") { *shape = {H, C}; return true; }
    if (name == "feature_projection.projection.bias") { *shape = {H}; return true; }
    if (name == "encoder.pos_conv_embed.conv.weight") { *shape = {H, H / c.pos_groups, c.pos_kernel}; return true; }
    if (name == "encoder.pos_conv_embed.conv.bias") { *shape = {H}; return true; }
    if (name == "encoder.layer_norm.weight" || name == "encoder.layer_norm.bias") { *shape = {H}; return true; }
    if (name.rfind("encoder.layers.", 0) != 0) return false;
    char* end = nullptr;
    const char* s = name.c_str() + 15;
    const long i = strtol(s, &end, 10);
    if (end == s || *end != '.' || i < 0 || i >= c.num_layers) return false;
    const std::string rest(end + 1);
    for (const char* p : {"attention.q_proj", "attention.k_proj", "attention.v_proj", "attention.out_proj"}) {
        if (rest == std::string(p) + ".weight") { *shape = {H, H}; return true; }
        if (rest == std::string(p) + ".bias") { *shape = {H}; return true; }
    }
    if (rest == "layer_norm.weight" || rest == "layer_norm.bias" || rest == "final_layer_norm.weight" || rest == "final_layer_norm.bias" ||
        rest == "feed_forward.output_dense.bias") { *shape = {H}; return true; }
    if (rest == "feed_forward.intermediate_dense.weight") { *shape = {F, H}; return true; }
    if (rest == "feed_forward.intermediate_dense.bias") { *shape = {F}; return true; }
    if (rest == "feed_forward.output_dense.weight") { *shape = {H, F}; return true; }
    return false;
}

std::vector<std::string> w2v_keys(const svi_w2v_config& c) {
    std::vector<std::string> k;
    for (int i = 0; i < W2V_CONVS; ++i) k.push_back("feature_extractor.conv_layers." + std::to_string(i) + ".conv.weight");
    for (const char* p : {"feature_extractor.conv_layers.0.layer_norm.weight", "feature_extractor.conv_layers.0.layer_norm.bias",
                          "feature_projection.layer_norm.weight", "feature_projection.layer_norm.bias", "feature_projection.projection.weight",
                          "feature_projection.projection.bias", "encoder.pos_conv_embed.conv.weight", "encoder.pos_conv_embed.conv.bias",
                          "encoder.layer_norm.weight", "encoder.layer_norm.bias"})
        k.push_back(p);
    const char* per[] = {"attention.q_proj.weight", "attention.q_proj.bias", "attention.k_proj.weight", "attention.k_proj.bias",
                         "attention.v_proj.weight", "attention.v_proj.bias", "attention.out_proj.weight", "attention.out_proj.bias",
                         "layer_norm.weight", "layer_norm.bias", "feed_forward.intermediate_dense.weight", "feed_forward.intermediate_dense.bias",
                         "feed_forward.output_dense.weight", "feed_forward.output_dense.bias", "final_layer_norm.weight", "final_layer_norm.bias"};
    for (int i = 0; i < c.num_layers; ++i)
        for (const char* p : per) k.push_back("encoder.layers." + std::to_string(i) + "." + p);
    return k;
}

svi_status w2v_grow(svi_w2v* h, size_t need) {
    if (h->ws_bytes >= need) return SVI_OK;
    if (h->ws) { SVI_CHECK_HIP(hipFree(h->ws)); h->ws = nullptr; h->ws_bytes = 0; }       // hipFree waits for the work that still reads it
    hipError_t e = hipMalloc((void**)&h->ws, need);
    if (e != hipSuccess) { svi_set_error("hipMalloc(%zu B audio encoder workspace) failed: %s", need, hipGetErrorString(e)); return SVI_ERR_OOM; }
    h->ws_bytes = need;
    return SVI_OK;
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
    const int chunks_wave = (int)((n + ST_CHUNK - 1) / ST_CHUNK), chunks_gn = (int)((T[1] + ST_CHUNK - 1) / ST_CHUNK);
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t s_wave = al((size_t)n * 4), s_a = al((size_t)T[1] * C * 4), s_b = al((size_t)T[2] * C * 4);
    const size_t s_part = al((size_t)std::max((size_t)chunks_wave, (size_t)chunks_gn * C) * 4), s_stat = al((size_t)2 * std::max(C, 1) * 4);
    const size_t s_sc = al((size_t)S * C * 4), s_sh = al((size_t)S * H * 4), s_sf = al((size_t)S * std::max(F, 3 * H) * 4);
    SVI_TRY(w2v_grow(h, s_wave + s_a + s_b + s_part + s_stat + 2 * s_sc + 4 * s_sh + s_sf));
    char* p = h->ws;
    float* Wv = reinterpret_cast<float*>(p); p += s_wave;
    float* A = reinterpret_cast<float*>(p); p += s_a;
    float* B = reinterpret_cast<float*>(p); p += s_b;
    float* Part = reinterpret_cast<float*>(p); p += s_part;
    float* Stat = reinterpret_cast<float*>(p); p += s_stat;
    float* I0 = reinterpret_cast<float*>(p); p += s_sc;
    float* I1 = reinterpret_cast<float*>(p); p += s_sc;
    float* X = reinterpret_cast<float*>(p); p += s_sh;
    float* Y = reinterpret_cast<float*>(p); p += s_sh;
    float* N1 = reinterpret_cast<float*>(p); p += s_sh;
    float* At = reinterpret_cast<float*>(p); p += s_sh;
    float* Big = reinterpret_cast<float*>(p);                       // q | k | v, then the feed-forward's hidden rows
    auto W = [&](const std::string& k) { return reinterpret_cast<const float*>(h->w[k].p); };
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
        a.w = W("feature_extractor.conv_layers." + std::to_string(i) + ".conv.weight");
        a.y = dst; a.ldy = C; a.Tout = T[i + 1];
        a.Cin_g = i == 0 ? 1 : C; a.Cout_g = C; a.groups = 1; a.k = W2V_KERNEL[i]; a.s = W2V_STRIDE[i]; a.pad = 0;
        a.gelu = i == 0 ? 0 : 1;                                      // layer 0: GroupNorm comes between the convolution and the GELU
        SVI_TRY(launch_conv1d(a, st));
        if (i == 0) {
            SVI_TRY(stats(dst, T[1], C));
            const long cnt = T[1] * C;
            hipLaunchKernelGGL(w2v_colnorm_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, (const float*)dst, dst, cnt, C, Stat, Stat + C,
                               W2V_GROUPNORM_EPS, W("feature_extractor.conv_layers.0.layer_norm.weight"),
                               W("feature_extractor.conv_layers.0.layer_norm.bias"), 1);
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
        SVI_TRY(svi_launch_enc_attention_f32(QKV, 3 * H, QKV + H, 3 * H, QKV + 2 * H, 3 * H, At, H, S, S, c.num_heads, D, scale, st));
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
    SVI_REQUIRE(D == 32 || D == 64 || D == 80 || D == 128, "svi_w2v_create: head dim %d (the encoder attention has 32, 64, 80, 128)", D);
    svi_w2v* h = new (std::nothrow) svi_w2v();
    if (!h) { svi_set_error("out of host memory"); return SVI_ERR_OOM; }
    h->cfg = *cfg;
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
    SVI_REQUIRE(h && name && dev_ptr && shape && rank >= 1 && rank <= 3, "svi_w2v_bind_weight: bad argument");
    SVI_REQUIRE(dtype == SVI_F32, "audio encoder parameter '%s' must be fp32 (the reference runs this model in fp32)", name);
    SVI_REQUIRE(((uintptr_t)dev_ptr % 16) == 0, "audio encoder parameter '%s' is not 16-byte aligned", name);
    std::vector<int64_t> want;
    bool used = true;
    if (!w2v_expected(h->cfg, name, &want, &used)) { svi_set_error("unknown audio encoder parameter '%s'", name); return SVI_ERR_INVALID; }
    if (!used) return SVI_OK;
    bool ok = (size_t)rank == want.size();
    for (int i = 0; ok && i < rank; ++i) ok = shape[i] == want[i];
    if (!ok) { svi_set_error("shape mismatch for audio encoder parameter '%s'", name); return SVI_ERR_INVALID; }
    Param q; q.p = dev_ptr; q.shape = want;
    h->w[name] = q;
    return SVI_OK;
}

extern "C" svi_status svi_w2v_check_bound(svi_w2v* h) {
    SVI_REQUIRE(h, "null handle");
    for (const auto& k : w2v_keys(h->cfg))
        if (!h->w.count(k)) { svi_set_error("audio encoder parameter '%s' was never bound", k.c_str()); return SVI_ERR_UNBOUND; }
    return SVI_OK;
}

extern "C" svi_status svi_w2v_set_max_frames(svi_w2v* h, int32_t max_frames) {
    SVI_REQUIRE(h, "svi_w2v_set_max_frames: null handle");
    SVI_REQUIRE(max_frames >= 1 && max_frames <= W2V_FRAME_CAP, "svi_w2v_set_max_frames: max_frames %d (1 .. %d)", max_frames, W2V_FRAME_CAP);
    h->max_frames = max_frames;
    return SVI_OK;
}

extern "C" svi_status svi_encoder_attention_f32(const float* Q, int32_t ldq, const float* K, int32_t ldk, const float* V, int32_t ldv, float* O, int32_t ldo,
                                                int32_t Lq, int32_t Lk, int32_t heads, int32_t D, float scale, int32_t kernel, svi_stream stream) {
    SVI_REQUIRE(Q && K && V && O, "svi_encoder_attention_f32: null argument");
    SVI_REQUIRE(D == 32 || D == 64 || D == 80 || D == 128, "svi_encoder_attention_f32: D %d (the encoder attention has 32, 64, 80, 128)", D);
    SVI_REQUIRE(heads >= 1 && heads <= 65535 && Lq >= 1 && Lk >= 1, "svi_encoder_attention_f32: heads %d (1 .. 65535), Lq %d, Lk %d (at least 1)", heads, Lq, Lk);
    SVI_REQUIRE(Lq <= W2V_FRAME_CAP, "svi_encoder_attention_f32: Lq %d is above the cap of %d rows", Lq, W2V_FRAME_CAP);
    SVI_REQUIRE(Lk <= W2V_FRAME_CAP, "svi_encoder_attention_f32: Lk %d is above the cap of %d keys", Lk, W2V_FRAME_CAP);
    const long row = (long)heads * D;
    SVI_REQUIRE(ldq >= row, "svi_encoder_attention_f32: ldq %d is smaller than heads * D = %ld", ldq, row);
    SVI_REQUIRE(ldk >= row, "svi_encoder_attention_f32: ldk %d is smaller than heads * D = %ld", ldk, row);
    SVI_REQUIRE(ldv >= row, "svi_encoder_attention_f32: ldv %d is smaller than heads * D = %ld", ldv, row);
    SVI_REQUIRE(ldo >= row, "svi_encoder_attention_f32: ldo %d is smaller than heads * D = %ld", ldo, row);
    SVI_REQUIRE((((uintptr_t)Q | (uintptr_t)K | (uintptr_t)V | (uintptr_t)O) & 3) == 0, "svi_encoder_attention_f32: operands must be 4-byte aligned");
    SVI_REQUIRE(kernel >= 0 && kernel <= 2, "svi_encoder_attention_f32: kernel %d (0: as the audio encoder launches, 1: resident, 2: streaming)", kernel);
    SVI_REQUIRE(kernel != 1 || Lk <= W2V_MAX_FRAMES, "svi_encoder_attention_f32: kernel 1 (resident) holds at most 2048 keys, Lk is %d", Lk);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (kernel == 2) return launch_enc_attention_stream(Q, ldq, K, ldk, V, ldv, O, ldo, Lq, Lk, heads, D, scale, st);
    if (kernel == 1) return launch_enc_attention<float, false>(Q, ldq, K, ldk, V, ldv, O, ldo, Lq, Lk, heads, D, scale, nullptr, nullptr, 0, st);
    return svi_launch_enc_attention_f32(Q, ldq, K, ldk, V, ldv, O, ldo, Lq, Lk, heads, D, scale, st);
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
