// svi_encoder_kernels.hip — the kernels the once-per-clip encoders share (svi_encoders.hip: umT5, CLIP; svi_wav2vec.hip: wav2vec2), each compiled here and
// nowhere else, behind the launchers svi_common.h declares: the encoder attention (resident: whole score rows in LDS, bf16 rounding points or plain fp32;
// streaming: any key count, fp32), nn.LayerNorm and the erf GELU in fp32.  svi_encoder_attention_f32 is the fp32 attention alone, as an operator.
//
// The sequences are at most 512 keys x 64 channels per head for the prompt-side encoders and the whole attention of either is < 2 % of its FLOP, so the
// resident kernel is a plain LDS-staged VALU kernel whose point is to restate the reference's rounding points exactly (scores rounded to bf16, bias added
// in bf16, softmax in fp32 over the whole row, NORMALISED probabilities rounded to bf16 before P.V) — which an online-softmax kernel cannot do.
#include <math.h>

#include "svi_encoder_host.h"

// the head sizes both attention kernels are instantiated for: one list for the two launch switches (svi_enc_head_dim_ok is its predicate)
#define ENC_HEAD_DIMS(CASE) CASE(32) CASE(64) CASE(80) CASE(128)

namespace {

template <typename T> __device__ __forceinline__ float ldf(const T* p);
template <> __device__ __forceinline__ float ldf<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float ldf<bf16>(const bf16* p) { return (float)*p; }

// One workgroup = one head x ENC_RQ query rows.  LDS: the query rows (fp32) and the full score rows (fp32).
//   BF16PTS: restate the bf16 module's rounding points (t5:73-76); otherwise plain fp32 (CLIP, SDPA in fp32).
//   bias:  emb[bucket_tab[key - query + tab_zero]][head]  (bf16 table [buckets][heads]) or none.
#define ENC_RQ 16
template <typename T, int D, bool BF16PTS>
__global__ __launch_bounds__(256) void enc_attention_kernel(const T* __restrict__ Q, int ldq, const T* __restrict__ K, int ldk,
                                                            const T* __restrict__ V, int ldv, T* __restrict__ O, int ldo, int Lq, int Lk,
                                                            float scale, const bf16* __restrict__ emb, int heads,
                                                            const int* __restrict__ bucket_tab, int tab_zero) {
    extern __shared__ __attribute__((aligned(16))) float enc_smem[];
    float* Qs = enc_smem;                       // [ENC_RQ][D]
    float* S = enc_smem + ENC_RQ * D;           // [ENC_RQ][Lk]
    const int tid = threadIdx.x, head = blockIdx.y, q0 = blockIdx.x * ENC_RQ;
    const int nq = min(ENC_RQ, Lq - q0);
    for (int i = tid; i < ENC_RQ * D; i += 256) {
        const int r = i / D, c = i - r * D;
        Qs[i] = r < nq ? ldf(Q + (size_t)(q0 + r) * ldq + head * D + c) : 0.f;
    }
    __syncthreads();
    // ---- scores: thread <-> key
    for (int j = tid; j < Lk; j += 256) {
        float acc[ENC_RQ];
#pragma unroll
        for (int r = 0; r < ENC_RQ; ++r) acc[r] = 0.f;
        const T* kp = K + (size_t)j * ldk + head * D;
#pragma unroll 4
        for (int c = 0; c < D; c += 4) {
            float kv[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) kv[e] = ldf(kp + c + e);
#pragma unroll
            for (int r = 0; r < ENC_RQ; ++r) {
                const f32x4 qv = *reinterpret_cast<const f32x4*>(Qs + r * D + c);
                acc[r] = fmaf(qv[0], kv[0], acc[r]); acc[r] = fmaf(qv[1], kv[1], acc[r]);
                acc[r] = fmaf(qv[2], kv[2], acc[r]); acc[r] = fmaf(qv[3], kv[3], acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < ENC_RQ; ++r) {
            float s = acc[r] * scale;
            if (BF16PTS) s = rbf(s);
            if (emb && r < nq) {                  // rows past the last query have no table entry (and no output)
                const float b = (float)emb[(size_t)bucket_tab[j - (q0 + r) + tab_zero] * heads + head];
                s += b;
                if (BF16PTS) s = rbf(s);
            }
            S[r * Lk + j] = s;
        }
    }
    __syncthreads();
    // ---- softmax over the whole row, fp32 (t5:75); wave w owns rows 4w..4w+3
    {
        const int lane = tid & 63, wave = tid >> 6;
        for (int r = 4 * wave; r < 4 * wave + 4; ++r) {
            float* row = S + r * Lk;
            float m = -INFINITY;
            for (int j = lane; j < Lk; j += 64) m = fmaxf(m, row[j]);
            m = wave_max(m);
            float sum = 0.f;
            for (int j = lane; j < Lk; j += 64) { const float e = expf(row[j] - m); row[j] = e; sum += e; }
            sum = wave_sum(sum);
            for (int j = lane; j < Lk; j += 64) { const float pr = row[j] / sum; row[j] = BF16PTS ? rbf(pr) : pr; }
        }
    }
    __syncthreads();
    // ---- O = P V: thread <-> (row group, channel); a V element is loaded once and used for all rows of the group
    constexpr int NG = 256 / D, RPG = (ENC_RQ + NG - 1) / NG;
    const int g = tid / D, c = tid - g * D;
    if (g < NG) {
        float acc[RPG];
#pragma unroll
        for (int r = 0; r < RPG; ++r) acc[r] = 0.f;
        const T* vp = V + head * D + c;
        for (int j = 0; j < Lk; ++j) {
            const float v = ldf(vp + (size_t)j * ldv);
#pragma unroll
            for (int r = 0; r < RPG; ++r) {
                const int row = g * RPG + r;
                if (row < ENC_RQ) acc[r] = fmaf(S[row * Lk + j], v, acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < RPG; ++r) {
            const int row = g * RPG + r;
            if (row < nq) O[(size_t)(q0 + row) * ldo + head * D + c] = (T)acc[r];
        }
    }
}

template <typename T, bool BF16PTS>
svi_status launch_enc_attention(const T* Q, int ldq, const T* K, int ldk, const T* V, int ldv, T* O, int ldo, int Lq, int Lk, int heads, int D,
                                float scale, const bf16* emb, const int* bucket_tab, int tab_zero, hipStream_t st) {
    SVI_REQUIRE(Lq > 0 && Lk > 0 && Lk <= SVI_ENC_RESIDENT_KEYS, "encoder attention: %d keys (supported: 1..2048)", Lk);
    const int lds = (ENC_RQ * D + ENC_RQ * Lk) * 4;
    dim3 grid((Lq + ENC_RQ - 1) / ENC_RQ, heads), block(256);
#define ENC_CASE(DD)                                                                                                               \
    case DD:                                                                                                                       \
        SVI_TRY(svi_ensure_lds(reinterpret_cast<const void*>(enc_attention_kernel<T, DD, BF16PTS>), 160 * 1024 - 256));              \
        hipLaunchKernelGGL((enc_attention_kernel<T, DD, BF16PTS>), grid, block, lds, st, Q, ldq, K, ldk, V, ldv, O, ldo, Lq, Lk, scale, \
                           emb, heads, bucket_tab, tab_zero);                                                                      \
        break;
    switch (D) {
        ENC_HEAD_DIMS(ENC_CASE)
        default: svi_set_error("encoder attention: head dim %d (supported: 32, 64, 80, 128)", D); return SVI_ERR_UNSUPPORTED;
    }
#undef ENC_CASE
    SVI_LAUNCH_CHECK();
    return SVI_OK;
}

// Everything below is compiled with floating-point contraction allowed, as it always was (these kernels used to follow the image encoder's preprocessing
// kernel, which ends with this pragma, in one translation unit); the resident attention above is not.  The committed fixtures are these bits.
#pragma clang fp contract(fast)

// nn.LayerNorm in fp32 (biased variance), one wave per row
__global__ __launch_bounds__(256) void layernorm_f32_kernel(const float* __restrict__ x, float* __restrict__ out, const float* __restrict__ w,
                                                            const float* __restrict__ b, int rows, int dim, float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* xp = x + (size_t)row * dim;
    float s = 0.f;
    for (int i = lane; i < dim; i += 64) s += xp[i];
    const float mean = wave_sum(s) / (float)dim;
    float q = 0.f;
    for (int i = lane; i < dim; i += 64) { const float d = xp[i] - mean; q = fmaf(d, d, q); }
    const float r = rsqrtf(wave_sum(q) / (float)dim + eps);
    float* op = out + (size_t)row * dim;
    for (int i = lane; i < dim; i += 64) op[i] = (xp[i] - mean) * r * w[i] + b[i];
}

__global__ void gelu_erf_f32_kernel(float* __restrict__ x, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = gelu_erf_f(x[i]);
}

// ---------------------------------------------------------------- streaming attention ----------------------------------------------
// The resident kernel's attention (ENC_RQ query rows per workgroup) for ANY key count, plain fp32 only — the audio encoder past 2048 frames.  The key
// axis is walked in tiles of ENC_KT keys and a query row keeps a running maximum m, a running sum l and an accumulator that is rescaled when the
// maximum moves (online softmax), so LDS and registers do not grow with Lk.  One workgroup = one head x ENC_RQ query rows, as there.  Per tile:
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
        ENC_HEAD_DIMS(ENC_CASE)
        default: svi_set_error("streaming encoder attention: head dim %d (supported: 32, 64, 80, 128)", D); return SVI_ERR_UNSUPPORTED;
    }
#undef ENC_CASE
    SVI_LAUNCH_CHECK();
    return SVI_OK;
}

}  // namespace

bool svi_enc_head_dim_ok(int D) { return D == 32 || D == 64 || D == 80 || D == 128; }

svi_status svi_launch_enc_attention_bf16(const bf16* Q, int ldq, const bf16* K, int ldk, const bf16* V, int ldv, bf16* O, int ldo, int Lq, int Lk, int heads,
                                         int D, float scale, const bf16* emb, const int* bucket_tab, int tab_zero, hipStream_t st) {
    return launch_enc_attention<bf16, true>(Q, ldq, K, ldk, V, ldv, O, ldo, Lq, Lk, heads, D, scale, emb, bucket_tab, tab_zero, st);
}
// SVI_ENC_ATT_AUTO: the resident kernel up to its 2048 keys — the same launch and the same bits as before there was a choice — and the streaming kernel above
svi_status svi_launch_enc_attention_f32(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, float* O, int ldo, int Lq, int Lk,
                                        int heads, int D, float scale, int kernel, hipStream_t st) {
    if (kernel == SVI_ENC_ATT_STREAM || (kernel == SVI_ENC_ATT_AUTO && Lk > SVI_ENC_RESIDENT_KEYS))
        return launch_enc_attention_stream(Q, ldq, K, ldk, V, ldv, O, ldo, Lq, Lk, heads, D, scale, st);
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

svi_status svi_enc_grow(EncHandle* h, size_t need) {
    if (h->ws_bytes >= need) return SVI_OK;
    if (h->ws) { SVI_CHECK_HIP(hipFree(h->ws)); h->ws = nullptr; h->ws_bytes = 0; }
    hipError_t e = hipMalloc((void**)&h->ws, need);
    if (e != hipSuccess) { svi_set_error("hipMalloc(%zu B %s workspace) failed: %s", need, h->w.noun, hipGetErrorString(e)); return SVI_ERR_OOM; }
    h->ws_bytes = need;
    return SVI_OK;
}

extern "C" svi_status svi_encoder_attention_f32(const float* Q, int32_t ldq, const float* K, int32_t ldk, const float* V, int32_t ldv, float* O, int32_t ldo,
                                                int32_t Lq, int32_t Lk, int32_t heads, int32_t D, float scale, int32_t kernel, svi_stream stream) {
    SVI_REQUIRE(Q && K && V && O, "svi_encoder_attention_f32: null argument");
    SVI_REQUIRE(svi_enc_head_dim_ok(D), "svi_encoder_attention_f32: D %d (the encoder attention has 32, 64, 80, 128)", D);
    SVI_REQUIRE(heads >= 1 && heads <= 65535 && Lq >= 1 && Lk >= 1, "svi_encoder_attention_f32: heads %d (1 .. 65535), Lq %d, Lk %d (at least 1)", heads, Lq, Lk);
    SVI_REQUIRE(Lq <= SVI_ENC_MAX_KEYS, "svi_encoder_attention_f32: Lq %d is above the cap of %d rows", Lq, SVI_ENC_MAX_KEYS);
    SVI_REQUIRE(Lk <= SVI_ENC_MAX_KEYS, "svi_encoder_attention_f32: Lk %d is above the cap of %d keys", Lk, SVI_ENC_MAX_KEYS);
    const long row = (long)heads * D;
    SVI_REQUIRE(ldq >= row, "svi_encoder_attention_f32: ldq %d is smaller than heads * D = %ld", ldq, row);
    SVI_REQUIRE(ldk >= row, "svi_encoder_attention_f32: ldk %d is smaller than heads * D = %ld", ldk, row);
    SVI_REQUIRE(ldv >= row, "svi_encoder_attention_f32: ldv %d is smaller than heads * D = %ld", ldv, row);
    SVI_REQUIRE(ldo >= row, "svi_encoder_attention_f32: ldo %d is smaller than heads * D = %ld", ldo, row);
    SVI_REQUIRE((((uintptr_t)Q | (uintptr_t)K | (uintptr_t)V | (uintptr_t)O) & 3) == 0, "svi_encoder_attention_f32: operands must be 4-byte aligned");
    SVI_REQUIRE(kernel >= 0 && kernel <= 2, "svi_encoder_attention_f32: kernel %d (0: as the audio encoder launches, 1: resident, 2: streaming)", kernel);
    SVI_REQUIRE(kernel != SVI_ENC_ATT_RESIDENT || Lk <= SVI_ENC_RESIDENT_KEYS, "svi_encoder_attention_f32: kernel 1 (resident) holds at most 2048 keys, Lk is %d", Lk);
    return svi_launch_enc_attention_f32(Q, ldq, K, ldk, V, ldv, O, ldo, Lq, Lk, heads, D, scale, kernel, reinterpret_cast<hipStream_t>(stream));
}
