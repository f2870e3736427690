// svi_lora.hip — LoRA merge into FP8-stored weights, and the fp32 -> e4m3fn cast it ends in (models/lora.py:231-264): the kernels and their
// two C ABI entry points (svi_lora_merge_e4m3, svi_f32_to_fp8_e4m3; include/svi_hip.h).
//
// When the model's parameters are float8_e4m3fn the reference merges in fp32 and re-quantises:
//     W <- e4m3fn( fp32(W) + alpha * mm( fp32(up), fp32(down) ) )
// with one fp32 rounding each for the product's sum, the scaling and the addition, and torch's cast at the end (svi_fp8.h).
// lora_merge_e4m3_kernel does that in place, one launch per matrix: W8 is read once and written once, everything else stays in registers.
//
// Work split.  A workgroup owns a 128 x 128 tile of W (2 x 2 waves of 64 x 64), a wave 4 x 4 tiles of v_mfma_f32_16x16x*.  The product is
// formed TRANSPOSED — MFMA rows are columns of W (operand A = rows of down^T), MFMA columns are rows of W (operand B = rows of up) — because
// the 16 x 16 accumulator keeps four consecutive MFMA rows per lane: with MFMA row 4 q + j of tile t standing for column 16 q + 4 t + j of the
// wave's 64, lane (q, n) ends up with sixteen CONSECUTIVE bytes of W's row n: one 16-byte load and one 16-byte store per lane and row tile.
// Which columns an MFMA row stands for is only a matter of which row of down^T the lane loads.
//
// Operand precision.  bf16 operands go to v_mfma_f32_16x16x32_bf16 (products exact, fp32 accumulation).  fp32 and fp16 operands are widened to
// fp32 and go to v_mfma_f32_16x16x4_f32, an exact fp32 fma chain: 1/16 of the bf16 rate, which makes an fp32-operand merge compute-bound
// (DESIGN.md), but nothing is split or truncated.
#include "svi_common.h"
#include "svi_fp8.h"

namespace {

typedef _Float16 f16;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;

// four consecutive k of an fp32 / fp16 operand row, widened
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 ld4(const f16* p) {
    const f16x4 h = *reinterpret_cast<const f16x4*>(p);
    return f32x4{(float)h.x, (float)h.y, (float)h.z, (float)h.w};
}

// four e4m3 codes (one dword of a W8 row) + the four fp32 products of the same columns -> the four merged codes
__device__ __forceinline__ unsigned merge4(unsigned w, f32x4 p, float alpha) {
    unsigned out = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float scaled = alpha * p[j];                                    // fp32 rounding point 2 (1 = the product's accumulation)
        const float sum = svi_e4m3fn_to_f32((w >> (8 * j)) & 0xffu) + scaled; // rounding point 3; -ffp-contract=off keeps the two apart
        out |= svi_f32_to_e4m3fn(sum) << (8 * j);
    }
    return out;
}

// up [out_f, r], down_t [in_f, r] (down transposed: both operands k-contiguous), w8 [out_f, in_f] e4m3fn codes, in place.
// in_f % 8 == 0, r % 8 == 0; w8 is 8-byte aligned, al16 = its rows are 16-byte aligned as well (base % 16 == 0 and in_f % 16 == 0).
template <typename T>
__global__ __launch_bounds__(256) void lora_merge_e4m3_kernel(unsigned char* __restrict__ w8, int out_f, int in_f, const T* __restrict__ up,
                                                              const T* __restrict__ down_t, int r, float alpha, int al16) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = lane & 15, q = lane >> 4;
    const int r0 = blockIdx.y * 128 + (wave >> 1) * 64, c0 = blockIdx.x * 128 + (wave & 1) * 64;
    if (r0 >= out_f || c0 >= in_f) return;                                    // a wave with nothing to do (no barriers in this kernel)

    // the operand rows this lane feeds; rows past the matrix are clamped (their results are never stored)
    const T* arow[4];
    const T* brow[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int col = c0 + 16 * (n >> 2) + 4 * t + (n & 3);
        arow[t] = down_t + (size_t)(col < in_f ? col : in_f - 1) * r;
        const int row = r0 + 16 * t + n;
        brow[t] = up + (size_t)(row < out_f ? row : out_f - 1) * r;
    }

    // lane (q, n) of the result: columns c0 + 16 q .. + 15 of rows r0 + 16 rt + n.  Their W8 bytes are requested NOW: the HBM round trip of the one stream
    // that bounds the launch runs under the operand loads and the matrix instructions.  in_f % 8 == 0: the two 8-byte halves are whole or absent.
    const int col = c0 + 16 * q;
    u32x4 w[4];
    bool h0[4], h1[4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
        const int row = r0 + 16 * rt + n;
        h0[rt] = row < out_f && col + 8 <= in_f;
        h1[rt] = row < out_f && col + 16 <= in_f;
        const unsigned char* p = w8 + (size_t)row * in_f + col;
        w[rt] = u32x4{0u, 0u, 0u, 0u};
        if (al16) {                                                           // in_f % 16 == 0: h0 == h1
            if (h1[rt]) w[rt] = *reinterpret_cast<const u32x4*>(p);
        } else {
            if (h0[rt]) { const u32x2 v = *reinterpret_cast<const u32x2*>(p); w[rt][0] = v[0]; w[rt][1] = v[1]; }
            if (h1[rt]) { const u32x2 v = *reinterpret_cast<const u32x2*>(p + 8); w[rt][2] = v[0]; w[rt][3] = v[1]; }
        }
    }

    f32x4 acc[4][4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[rt][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    if constexpr (__is_same(T, bf16)) {
        // bf16: 32 k per instruction, lane quarter q holds k = kb + 8 q .. + 7 of its row; a quarter past r contributes zeros
        for (int kb = 0; kb < r; kb += 32) {
            const int k = kb + 8 * q;
            const bool live = k < r;
            bf16x8 a[4], b[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                a[t] = live ? ld_bf16x8(arow[t] + k) : bf16x8{};
                b[t] = live ? ld_bf16x8(brow[t] + k) : bf16x8{};
            }
#pragma unroll
            for (int rt = 0; rt < 4; ++rt)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[rt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t], b[rt], acc[rt][t], 0, 0, 0);
        }
    } else {
        // fp32 / fp16 (widened): 4 k per instruction, one per lane quarter.  A lane loads k = kb + 4 q .. + 3 at once and instruction m takes
        // its element m — the four instructions of a 16-k group cover the group once, in an order of their own (any order is inside the bound)
        for (int kb = 0; kb < r; kb += 16) {
            const int k = kb + 4 * q;
            const bool live = k < r;
            f32x4 a[4], b[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                a[t] = live ? ld4(arow[t] + k) : f32x4{0.f, 0.f, 0.f, 0.f};
                b[t] = live ? ld4(brow[t] + k) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int rt = 0; rt < 4; ++rt)
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[rt][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][m], b[rt][m], acc[rt][t], 0, 0, 0);
        }
    }

    // dword t of a lane's sixteen bytes = acc[rt][t]
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
#pragma unroll
        for (int t = 0; t < 4; ++t) w[rt][t] = merge4(w[rt][t], acc[rt][t], alpha);
        unsigned char* p = w8 + (size_t)(r0 + 16 * rt + n) * in_f + col;
        if (al16) {
            if (h1[rt]) *reinterpret_cast<u32x4*>(p) = w[rt];
        } else {
            if (h0[rt]) *reinterpret_cast<u32x2*>(p) = u32x2{w[rt][0], w[rt][1]};
            if (h1[rt]) *reinterpret_cast<u32x2*>(p + 8) = u32x2{w[rt][2], w[rt][3]};
        }
    }
}

// out e4m3fn [n] = cast(in [n]); eight elements per thread where both pointers allow vector access (vec), the tail one by one
template <typename T>
__global__ __launch_bounds__(256) void f32_to_fp8_e4m3_kernel(const T* __restrict__ in, unsigned char* __restrict__ out, int64_t n, int vec) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
    if (i >= n) return;
    if (vec && i + 8 <= n) {
        float v[8];
        if constexpr (sizeof(T) == 4) {
            const f32x4 lo = *reinterpret_cast<const f32x4*>(in + i), hi = *reinterpret_cast<const f32x4*>(in + i + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[e] = lo[e]; v[4 + e] = hi[e]; }
        } else {
            const bf16x8 x = ld_bf16x8(reinterpret_cast<const bf16*>(in + i));
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (float)x[e];
        }
        u32x2 w{0u, 0u};
#pragma unroll
        for (int e = 0; e < 8; ++e) w[e >> 2] |= svi_f32_to_e4m3fn(v[e]) << (8 * (e & 3));
        *reinterpret_cast<u32x2*>(out + i) = w;
    } else {
        for (int64_t e = i; e < n && e < i + 8; ++e) out[e] = (unsigned char)svi_f32_to_e4m3fn((float)in[e]);
    }
}

template <typename T>
svi_status launch_merge(unsigned char* w8, int out_f, int in_f, const void* up, const void* down_t, int r, float alpha, hipStream_t st) {
    const int al16 = (reinterpret_cast<uintptr_t>(w8) % 16 == 0 && in_f % 16 == 0) ? 1 : 0;
    hipLaunchKernelGGL(lora_merge_e4m3_kernel<T>, dim3((unsigned)((in_f + 127) / 128), (unsigned)((out_f + 127) / 128)), dim3(256), 0, st, w8, out_f, in_f,
                       reinterpret_cast<const T*>(up), reinterpret_cast<const T*>(down_t), r, alpha, al16);
    SVI_LAUNCH_CHECK();
    return SVI_OK;
}

}  // namespace

extern "C" svi_status svi_f32_to_fp8_e4m3(const void* in, svi_dtype in_dtype, void* out, int64_t n, svi_stream stream) {
    SVI_REQUIRE(in && out && n >= 0, "svi_f32_to_fp8_e4m3: bad argument");
    SVI_REQUIRE(in_dtype == SVI_F32 || in_dtype == SVI_BF16, "svi_f32_to_fp8_e4m3: input must be fp32 or bf16 (got dtype %d)", (int)in_dtype);
    if (n == 0) return SVI_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    unsigned char* o = reinterpret_cast<unsigned char*>(out);
    const int vec = (reinterpret_cast<uintptr_t>(in) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 8 == 0) ? 1 : 0;
    const int64_t blocks = (n + 2047) / 2048;
    SVI_REQUIRE(blocks < (1LL << 31), "svi_f32_to_fp8_e4m3: n = %lld is beyond one launch", (long long)n);
    const dim3 grid((unsigned)blocks);
    if (in_dtype == SVI_BF16) hipLaunchKernelGGL(f32_to_fp8_e4m3_kernel<bf16>, grid, dim3(256), 0, st, reinterpret_cast<const bf16*>(in), o, n, vec);
    else hipLaunchKernelGGL(f32_to_fp8_e4m3_kernel<float>, grid, dim3(256), 0, st, reinterpret_cast<const float*>(in), o, n, vec);
    SVI_LAUNCH_CHECK();
    return SVI_OK;
}

extern "C" svi_status svi_lora_merge_e4m3(void* w8, int32_t out_f, int32_t in_f, const void* up, const void* down_t, svi_dtype dtype, int32_t r, float alpha,
                                          svi_stream stream) {
    SVI_REQUIRE(w8 && up && down_t, "svi_lora_merge_e4m3: null argument");
    SVI_REQUIRE(dtype == SVI_BF16 || dtype == SVI_F16 || dtype == SVI_F32, "svi_lora_merge_e4m3: operands must be bf16, fp16 or fp32 (got dtype %d)", (int)dtype);
    SVI_REQUIRE(out_f >= 0 && in_f >= 0 && r > 0, "svi_lora_merge_e4m3: bad shape [%d, %d], rank %d", out_f, in_f, r);
    SVI_REQUIRE(in_f % 8 == 0 && r % 8 == 0, "svi_lora_merge_e4m3: in_features (%d) and rank (%d) must be multiples of 8", in_f, r);
    SVI_REQUIRE((out_f + 127) / 128 <= 65535, "svi_lora_merge_e4m3: out_features (%d) is beyond one launch", out_f);
    SVI_REQUIRE(reinterpret_cast<uintptr_t>(w8) % 8 == 0, "svi_lora_merge_e4m3: the weight must be 8-byte aligned");
    SVI_REQUIRE(reinterpret_cast<uintptr_t>(up) % 16 == 0 && reinterpret_cast<uintptr_t>(down_t) % 16 == 0, "svi_lora_merge_e4m3: the operands must be 16-byte aligned");
    if (out_f == 0 || in_f == 0) return SVI_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    unsigned char* w = reinterpret_cast<unsigned char*>(w8);
    switch (dtype) {
        case SVI_BF16: return launch_merge<bf16>(w, out_f, in_f, up, down_t, r, alpha, st);
        case SVI_F16: return launch_merge<f16>(w, out_f, in_f, up, down_t, r, alpha, st);
        default: return launch_merge<float>(w, out_f, in_f, up, down_t, r, alpha, st);
    }
}
