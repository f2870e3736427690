// svi_elementwise.hip — HBM-bound row kernels of the DiT block (gfx950).
//
// All of these stream a [rows, dim] bf16 activation once: one 64-lane wave owns one row, each lane
// holds 16-byte (8 x bf16) chunks of it in registers, statistics are reduced across the wave, and
// the row is written once.  Algorithmic traffic = 2 * rows * dim * 2 bytes (read + write); that is
// the figure the roofline fraction of these kernels is quoted against.
//
// Rounding: the reference runs these ops as separate bf16 tensor ops; `rbf()` marks each point
// where it materialises a bf16 tensor so results track it to within accumulation-order noise.
#include "svi_common.h"
#include <type_traits>

#define ROWS_PER_BLOCK 4      // 4 waves / 256 threads per workgroup

// A kernel is built for MAXC chunks per lane: 3 (up to 1536 columns, the 1.3B width), 10 (up to 5120, the 14B width) or 16 (up to 8192).
// launch(std::integral_constant<int, MAXC>) instantiates and launches; the one place the widths are mapped.
template <class F>
static void with_maxc(int nchunk, F&& launch) {
    if (nchunk <= 64 * 3) launch(std::integral_constant<int, 3>{});
    else if (nchunk <= 64 * 10) launch(std::integral_constant<int, 10>{});
    else launch(std::integral_constant<int, 16>{});
}
constexpr int RPW = 4;        // rows a wave of the multi-row kernels walks (they exist for rows of 3 and of 10 whole chunks per lane)

// grid of the grid-stride 1-D kernels: 256 elements per workgroup, at most `cap` workgroups
static dim3 grid_1d(int64_t n, int cap) { return dim3((unsigned)((n + 255) / 256 < cap ? (n + 255) / 256 : cap)); }

// ------------------------------------------------------------------------------------------------
// LayerNorm (no affine | affine) [+ modulate]:  out = ((x-mean)*rstd [*w+b]) [*(1+scale)+shift]
// reference: nn.LayerNorm(eps=1e-6) + modulate(), models/wan_video_dit.py:150-151,331-333,358,370,372
//
// The row body.  ln_mod_kernel and add_ln_mod_skip_kernel both call ln_row_stats and ln_emit_chunk on a wave's row held as float v[MAXC][8] and the
// project builds with -ffp-contract=off, so their results cannot diverge: a row has the same bits whichever of them wrote it.  ln_mod_rows_kernel keeps
// the same statements written out (see there).
// ------------------------------------------------------------------------------------------------
// FULL: every lane holds MAXC whole chunks (no guards); otherwise chunk lane + 64 c exists while it is below nchunk.
template <int MAXC, bool FULL>
__device__ __forceinline__ void ln_row_stats(const float (&v)[MAXC][8], int lane, int nchunk, int dim, float eps, float& mean, float& rstd) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (FULL || lane + 64 * c < nchunk) {
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[c][j];
        }
    mean = wave_sum(s) / (float)dim;
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (FULL || lane + 64 * c < nchunk) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { float d = v[c][j] - mean; q += d * d; }
        }
    rstd = rsqrtf(wave_sum(q) / (float)dim + eps);
}

// the affine and modulation vectors of one chunk (columns col .. col + 7); a part that is not asked for is left unset and never read
struct LnVecs { bf16x8 w, b; f32x4 sc[2], sh[2]; };
__device__ __forceinline__ LnVecs ln_load_vecs(bool affine, bool mod, const bf16* __restrict__ w, const bf16* __restrict__ b, const float* __restrict__ shift,
                                               const float* __restrict__ scale1p, int col) {
    LnVecs p;
    if (affine) { p.w = ld_bf16x8(w + col); p.b = ld_bf16x8(b + col); }
    if (mod) {
        p.sc[0] = *reinterpret_cast<const f32x4*>(scale1p + col); p.sc[1] = *reinterpret_cast<const f32x4*>(scale1p + col + 4);
        p.sh[0] = *reinterpret_cast<const f32x4*>(shift + col); p.sh[1] = *reinterpret_cast<const f32x4*>(shift + col + 4);
    }
    return p;
}
// affine / mod are compile-time constants in the kernels that are templated on them and wave-uniform flags in ln_mod_kernel
__device__ __forceinline__ bf16x8 ln_emit_chunk(const float (&v)[8], float mean, float rstd, bool affine, bool mod, const LnVecs& p) {
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float y = (v[j] - mean) * rstd;
        if (affine) y = y * (float)p.w[j] + (float)p.b[j];
        y = rbf(y);
        if (mod) y = rbf(rbf(y * p.sc[j >> 2][j & 3]) + p.sh[j >> 2][j & 3]);
        o[j] = (bf16)y;
    }
    return o;
}

// generic: one row per wave, any dim that is a multiple of 8
template <int MAXC>
__global__ __launch_bounds__(256) void ln_mod_kernel(const bf16* __restrict__ x, int ldx, bf16* __restrict__ out, int ldo, int rows, int dim, float eps,
                                                     const bf16* __restrict__ w, const bf16* __restrict__ b, const float* __restrict__ shift, const float* __restrict__ scale1p) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nchunk = dim >> 3;
    const bf16* xr = x + (size_t)row * ldx;
    float v[MAXC][8];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const int ci = lane + 64 * c;
        bf16x8 t = {};
        if (ci < nchunk) t = ld_bf16x8(xr + ci * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[c][j] = (float)t[j];
    }
    float mean, rstd;
    ln_row_stats<MAXC, false>(v, lane, nchunk, dim, eps, mean, rstd);
    bf16* orow = out + (size_t)row * ldo;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const int ci = lane + 64 * c;
        if (ci < nchunk) st_bf16x8(orow + ci * 8, ln_emit_chunk(v[c], mean, rstd, w != nullptr, scale1p != nullptr, ln_load_vecs(w != nullptr, scale1p != nullptr, w, b, shift, scale1p, ci * 8)));
    }
}

// Rows of whole chunks (dim = 512 MAXC): a wave walks RPW consecutive rows with row i + 1 requested before row i is worked on; for MAXC <= 3 (the 1.3B
// width) the modulation / affine vectors stay in registers instead of being reloaded for every row.  The arithmetic is the row body's, written out:
// built on ln_row_stats / ln_emit_chunk the compiler schedules this kernel differently and the step's LayerNorm time rose by 0.7 % (5.64 -> 5.68 ms,
// profiles/row_body_ab.txt).  tests/test_gpu_row_kernels.py holds it to ln_mod_kernel bit for bit.
template <int MAXC, int RPW, bool AFFINE, bool MOD>
__global__ __launch_bounds__(256) void ln_mod_rows_kernel(const bf16* __restrict__ x, int ldx, bf16* __restrict__ out, int ldo, int rows, int dim, float eps,
                                                          const bf16* __restrict__ w, const bf16* __restrict__ b, const float* __restrict__ shift,
                                                          const float* __restrict__ scale1p) {
    constexpr bool HOIST = MAXC <= 3;
    const int lane = threadIdx.x & 63;
    const int row0 = (blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6)) * RPW;
    if (row0 >= rows) return;
    const int row_end = min(rows, row0 + RPW);
    bf16x8 cur[MAXC], nxt[MAXC];
    bf16x8 wv[HOIST ? MAXC : 1], bv[HOIST ? MAXC : 1];
    f32x4 sc[HOIST ? MAXC : 1][2], sh[HOIST ? MAXC : 1][2];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const int col = (lane + 64 * c) * 8;
        cur[c] = ld_bf16x8(x + (size_t)row0 * ldx + col);
        nxt[c] = cur[c];
        if constexpr (HOIST) {
            if constexpr (AFFINE) { wv[c] = ld_bf16x8(w + col); bv[c] = ld_bf16x8(b + col); }
            if constexpr (MOD) {
                sc[c][0] = *reinterpret_cast<const f32x4*>(scale1p + col); sc[c][1] = *reinterpret_cast<const f32x4*>(scale1p + col + 4);
                sh[c][0] = *reinterpret_cast<const f32x4*>(shift + col); sh[c][1] = *reinterpret_cast<const f32x4*>(shift + col + 4);
            }
        }
    }
    for (int row = row0; row < row_end; ++row) {
        if (row + 1 < row_end) {
#pragma unroll
            for (int c = 0; c < MAXC; ++c) nxt[c] = ld_bf16x8(x + (size_t)(row + 1) * ldx + (lane + 64 * c) * 8);
        }
        float v[MAXC][8];
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
#pragma unroll
            for (int j = 0; j < 8; ++j) { v[c][j] = (float)cur[c][j]; s += v[c][j]; }
        const float mean = wave_sum(s) / (float)dim;
        float q = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
#pragma unroll
            for (int j = 0; j < 8; ++j) { float d = v[c][j] - mean; q += d * d; }
        const float rstd = rsqrtf(wave_sum(q) / (float)dim + eps);
        bf16* orow = out + (size_t)row * ldo;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            const int col = (lane + 64 * c) * 8;
            bf16x8 wc, bc;
            f32x4 sc0, sc1, sh0, sh1;
            if constexpr (HOIST) {
                if constexpr (AFFINE) { wc = wv[c]; bc = bv[c]; }
                if constexpr (MOD) { sc0 = sc[c][0]; sc1 = sc[c][1]; sh0 = sh[c][0]; sh1 = sh[c][1]; }
            } else {
                if constexpr (AFFINE) { wc = ld_bf16x8(w + col); bc = ld_bf16x8(b + col); }
                if constexpr (MOD) {
                    sc0 = *reinterpret_cast<const f32x4*>(scale1p + col); sc1 = *reinterpret_cast<const f32x4*>(scale1p + col + 4);
                    sh0 = *reinterpret_cast<const f32x4*>(shift + col); sh1 = *reinterpret_cast<const f32x4*>(shift + col + 4);
                }
            }
            bf16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float y = (v[c][j] - mean) * rstd;
                if constexpr (AFFINE) y = y * (float)wc[j] + (float)bc[j];
                y = rbf(y);
                if constexpr (MOD) y = rbf(rbf(y * (j < 4 ? sc0[j & 3] : sc1[j & 3])) + (j < 4 ? sh0[j & 3] : sh1[j & 3]));
                o[j] = (bf16)y;
            }
            st_bf16x8(orow + col, o);
        }
#pragma unroll
        for (int c = 0; c < MAXC; ++c) cur[c] = nxt[c];
    }
}

svi_status svi_launch_ln_mod(const bf16* x, int ldx, bf16* out, int ldo, int rows, int dim, float eps,
                             const bf16* w, const bf16* b, const float* shift, const float* scale1p, hipStream_t st) {
    SVI_REQUIRE(dim % 8 == 0 && ldx % 8 == 0 && ldo % 8 == 0, "layernorm: dim/ld must be multiples of 8 (dim=%d)", dim);
    SVI_REQUIRE(dim <= 8192, "layernorm: dim %d > 8192 unsupported", dim);
    SVI_REQUIRE((w == nullptr) == (b == nullptr), "layernorm: affine weight and bias must come together");
    SVI_REQUIRE((shift == nullptr) == (scale1p == nullptr), "layernorm: shift and scale must come together");
    if (rows <= 0) return SVI_OK;
    dim3 grid((rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK), block(256);
    const int nchunk = dim / 8;
    // the DiT's widths (whole chunks per lane) and norm kinds (modulated without affine: norm1 / norm2; affine without modulation: norm3): the
    // multi-row kernel.  The modulation vectors must be 16-byte aligned for its vector loads (the DiT's are).
    const bool multi_row = (nchunk == 64 * 3 || nchunk == 64 * 10) && svi_switches().rms_rows && ((w != nullptr) != (scale1p != nullptr)) &&
                           ((((uintptr_t)shift | (uintptr_t)scale1p) & 15) == 0);
    const dim3 grid_r((rows + ROWS_PER_BLOCK * RPW - 1) / (ROWS_PER_BLOCK * RPW));
    with_maxc(nchunk, [&](auto mc) {
        constexpr int MAXC = decltype(mc)::value;
        if constexpr (MAXC <= 10) {
            if (multi_row && w) { hipLaunchKernelGGL((ln_mod_rows_kernel<MAXC, RPW, true, false>), grid_r, block, 0, st, x, ldx, out, ldo, rows, dim, eps, w, b, shift, scale1p); return; }
            if (multi_row) { hipLaunchKernelGGL((ln_mod_rows_kernel<MAXC, RPW, false, true>), grid_r, block, 0, st, x, ldx, out, ldo, rows, dim, eps, w, b, shift, scale1p); return; }
        }
        hipLaunchKernelGGL(ln_mod_kernel<MAXC>, grid, block, 0, st, x, ldx, out, ldo, rows, dim, eps, w, b, shift, scale1p);
    });
    SVI_LAUNCH_CHECK();
    return SVI_OK;
}

// ------------------------------------------------------------------------------------------------
// RMSNorm over the full model dim (all heads jointly) [+ 3-D RoPE per head], in place.
// reference: RMSNorm.forward models/wan_video_dit.py:192-197; rope_apply :178-183 with the table of
// :161-175 gathered per token at pipelines/svi_video.py:106-110.  The reference rotates in fp64;
// here cos/sin come from a host-built fp64->fp32 table and the 2x2 rotate runs in fp32 — the result
// is rounded to bf16 either way (difference <= 1 bf16 ulp on rounding ties only).
// ------------------------------------------------------------------------------------------------
// The row body.  rmsnorm_rope_kernel and rmsnorm_rope_rows_kernel both call rms_row_rs and rms_emit_chunk, so their results cannot diverge (FULL as above).
template <int MAXC, bool FULL>
__device__ __forceinline__ float rms_row_rs(const float (&v)[MAXC][8], int lane, int nchunk, int dim, float eps) {
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (FULL || lane + 64 * c < nchunk) {
#pragma unroll
            for (int j = 0; j < 8; ++j) ss += v[c][j] * v[c][j];
        }
    return rsqrtf(wave_sum(ss) / (float)dim + eps);
}
// one chunk: normalise, gain, [rotate its four complex pairs by (cx[p], sy[p]) = (cos, sin)], scale
__device__ __forceinline__ bf16x8 rms_emit_chunk(const float (&v)[8], float rs, bf16x8 gain, bool rope, const float (&cx)[4], const float (&sy)[4], float out_scale) {
    float y[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = rbf(rbf(v[j] * rs) * (float)gain[j]);
    bf16x8 o;
    if (rope) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const float a = y[2 * p], bq = y[2 * p + 1];
            o[2 * p] = (bf16)((a * cx[p] - bq * sy[p]) * out_scale);
            o[2 * p + 1] = (bf16)((a * sy[p] + bq * cx[p]) * out_scale);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (bf16)(y[j] * out_scale);
    }
    return o;
}
// the four (cos, sin) pairs at tt[0 .. 3] of a token's table row
__device__ __forceinline__ void rope_pairs_of(const float2* tt, float (&cx)[4], float (&sy)[4]) {
    const f32x4 t01 = *reinterpret_cast<const f32x4*>(tt), t23 = *reinterpret_cast<const f32x4*>(tt + 2);
    cx[0] = t01[0]; cx[1] = t01[2]; cx[2] = t23[0]; cx[3] = t23[2];
    sy[0] = t01[1]; sy[1] = t01[3]; sy[2] = t23[1]; sy[3] = t23[3];
}

// blockIdx.y selects one of up to two [rows, dim] operands that sit side by side in a row (q | k of the DiT's QK buffer): operand
// p starts at column p * dim and has its own weight and output scale — one launch normalises both.
// generic: one row per wave, any dim that is a multiple of 8; RoPE from the per-token table or the three axis tables; in place or to SviScatter
template <int MAXC, bool SCATTER>
__global__ __launch_bounds__(256) void rmsnorm_rope_kernel(bf16* __restrict__ x, int ld, int rows, int dim, const bf16* __restrict__ weight,
                                                           const bf16* __restrict__ weight1, float eps, int use_rope, SviRope r, float out_scale, float out_scale1, SviScatter sc) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nchunk = dim >> 3;
    bf16* xr = x + (size_t)row * ld + (size_t)blockIdx.y * dim;
    if (blockIdx.y) { weight = weight1; out_scale = out_scale1; }
    float v[MAXC][8];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const int ci = lane + 64 * c;
        if (ci < nchunk) {
            bf16x8 t = ld_bf16x8(xr + ci * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[c][j] = (float)t[j];
        }
    }
    const float rs = rms_row_rs<MAXC, false>(v, lane, nchunk, dim, eps);
    int pf = 0, ph = 0, pw = 0;
    const float2* tt = nullptr;                  // this token's 64 pairs, when the caller gathered them (SviRope::tab_tok)
    if (use_rope) {
        const int hw = r.h * r.w;
        int tok = row;
        if (r.period > 0) tok %= r.period;
        tok += r.row0;
        if (r.tab_tok) tt = r.tab_tok + (size_t)tok * 64;
        pf = tok / hw;
        const int rem = tok - pf * hw;
        ph = rem / r.w;
        pw = rem - ph * r.w;
    }
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const int ci = lane + 64 * c;
        if (ci < nchunk) {
            const int col = ci * 8;
            float cx[4], sy[4];
            if (use_rope) {
                const int pair0 = (col & 127) >> 1;            // complex-pair index inside the head
                if (tt) rope_pairs_of(tt + pair0, cx, sy);
                else {
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const int pi = pair0 + p;
                        float2 cs;
                        if (pi < r.npf) cs = r.tab_f[pf * r.npf + pi];
                        else if (pi < r.npf + r.nph) cs = r.tab_h[ph * r.nph + (pi - r.npf)];
                        else cs = r.tab_w[pw * r.npw + (pi - r.npf - r.nph)];
                        cx[p] = cs.x; sy[p] = cs.y;
                    }
                }
            }
            const bf16x8 o = rms_emit_chunk(v[c], rs, ld_bf16x8(weight + col), use_rope != 0, cx, sy, out_scale);
            if constexpr (SCATTER) {
                const int j = col / sc.Dp, cl = col - j * sc.Dp, gq = cl / sc.Dg, cg = cl - gq * sc.Dg;
                bf16* ob = blockIdx.y ? sc.out1 : sc.out0;
                int rps = rows, rr = row, nbr = 1, smp = 0;
                if (sc.rows_per_sample > 0) { rps = sc.rows_per_sample; nbr = rows / rps; smp = row / rps; rr = row - smp * rps; }
                st_bf16x8(ob + (((size_t)(gq * sc.P + j) * rps + rr) * nbr + smp) * sc.Dg + cg, o);
            } else {
                st_bf16x8(xr + col, o);
            }
        }
    }
}

// The shapes the DiT runs (every lane holds MAXC whole chunks: dim = 512 MAXC; RoPE from the per-token table or none; in place): a wave walks RPW
// consecutive rows, requests row i + 1 before it works on row i, and keeps the gain vector in registers — the generic kernel above reloads and unpacks
// it for every row and has one row in flight per wave.
// Q8 (opt-in fp8 QK^T attention): the result rows leave as MX e4m3 bytes + E8M0 block scales (operand blockIdx.y -> q8o.q8 / q8o.k8) instead of bf16 —
// a lane's 8 channels are a quarter of a 32-channel block and 16 lanes one head: the quantiser's own lane layout (mx8_quant8), so the bits are those
// svi_launch_mx8_quantize makes of the bf16 rows this kernel would have written.
template <int MAXC, int RPW, bool ROPE, bool Q8 = false>
__global__ __launch_bounds__(256) void rmsnorm_rope_rows_kernel(bf16* __restrict__ x, int ld, int rows, int dim, const bf16* __restrict__ weight,
                                                                const bf16* __restrict__ weight1, float eps, SviRope r, float out_scale, float out_scale1, SviQk8 q8o = SviQk8{}) {
    const int lane = threadIdx.x & 63;
    const int row0 = (blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6)) * RPW;
    if (row0 >= rows) return;
    const int row_end = min(rows, row0 + RPW);
    bf16* xb = x + (size_t)blockIdx.y * dim;
    if (blockIdx.y) { weight = weight1; out_scale = out_scale1; }
    bf16x8 wv[MAXC], cur[MAXC], nxt[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        wv[c] = ld_bf16x8(weight + (lane + 64 * c) * 8);
        cur[c] = ld_bf16x8(xb + (size_t)row0 * ld + (lane + 64 * c) * 8);
        nxt[c] = cur[c];
    }
    for (int row = row0; row < row_end; ++row) {
        if (row + 1 < row_end) {
#pragma unroll
            for (int c = 0; c < MAXC; ++c) nxt[c] = ld_bf16x8(xb + (size_t)(row + 1) * ld + (lane + 64 * c) * 8);
        }
        float v[MAXC][8];
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
#pragma unroll
            for (int j = 0; j < 8; ++j) v[c][j] = (float)cur[c][j];
        const float rs = rms_row_rs<MAXC, true>(v, lane, MAXC * 64, dim, eps);
        const float2* tt = nullptr;
        if (ROPE) {
            int tok = row;
            if (r.period > 0) tok %= r.period;
            tok += r.row0;
            tt = r.tab_tok + (size_t)tok * 64;
        }
        bf16* xr = xb + (size_t)row * ld;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            const int col = (lane + 64 * c) * 8;
            float cx[4], sy[4];
            if (ROPE) rope_pairs_of(tt + ((col & 127) >> 1), cx, sy);
            const bf16x8 o = rms_emit_chunk(v[c], rs, wv[c], ROPE, cx, sy, out_scale);
            if constexpr (Q8) {
                float vq[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) vq[j] = (float)o[j];
                mx8_quant8(vq, true, row, lane + 64 * c, blockIdx.y ? q8o.k8 : q8o.q8, q8o.ld8, blockIdx.y ? q8o.ks : q8o.qs, blockIdx.y ? q8o.ks_rows : q8o.qs_rows);
            } else {
                st_bf16x8(xr + col, o);
            }
        }
#pragma unroll
        for (int c = 0; c < MAXC; ++c) cur[c] = nxt[c];
    }
}

// rs[m] = rsqrt(mean_n q[m][n]^2 + eps) from the per-64-column sums of squares the q projection's epilogue left (SviGemmArgs::rowss): groups summed in
// index order; the division and the rsqrt are rmsnorm_rope_kernel's.  flash_cross_kernel applies the normalisation as it reads q.
__global__ __launch_bounds__(256) void row_rs_kernel(const float* __restrict__ rowss, int groups, int ldss, int rows, float dim, float eps, float* __restrict__ rs) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= rows) return;
    float ss = 0.f;
    int g = 0;
    for (; g + 8 <= groups; g += 8) {          // eight loads in flight, added in index order
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = rowss[(size_t)(g + i) * ldss + m];
#pragma unroll
        for (int i = 0; i < 8; ++i) ss += v[i];
    }
    for (; g < groups; ++g) ss += rowss[(size_t)g * ldss + m];
    rs[m] = rsqrtf(ss / dim + eps);
}
svi_status svi_launch_row_rs(const float* rowss, int groups, int ldss, int rows, int dim, float eps, float* rs, hipStream_t st) {
    SVI_REQUIRE(rowss && rs && groups > 0 && groups * 64 == dim && ldss >= rows, "row_rs: bad layout (groups %d, dim %d, ldss %d, rows %d)", groups, dim, ldss, rows);
    if (rows <= 0) return SVI_OK;
    hipLaunchKernelGGL(row_rs_kernel, dim3((rows + 63) / 64), dim3(64), 0, st, rowss, groups, ldss, rows, (float)dim, eps, rs);      // (1024 workgroups at the C2 size: every CU busy)
    SVI_LAUNCH_CHECK();
    return SVI_OK;
}

bool svi_rmsnorm_rope_q8_ok(int dim, const SviRope* rope) {
    return (dim == 512 * 3 || dim == 512 * 10) && rope && rope->tab_tok && svi_switches().rms_rows;
}
svi_status svi_launch_rmsnorm_rope2_q8(bf16* x, int ld, int rows, int dim, const bf16* weight, const bf16* weight1, float eps, const SviRope* rope, float out_scale,
                                       float out_scale1, hipStream_t st, const SviQk8& out) {
    SVI_REQUIRE(svi_rmsnorm_rope_q8_ok(dim, rope) && weight1 && ld >= 2 * dim && ld % 8 == 0, "rmsnorm -> e4m3: only the DiT's q | k launch (dim %d)", dim);
    SVI_REQUIRE(out.q8 && out.k8 && out.qs && out.ks && out.ld8 >= dim && out.ld8 % 8 == 0 && out.qs_rows >= rows && out.ks_rows >= rows, "rmsnorm -> e4m3: bad output buffers");
    SVI_REQUIRE(rope->npf + rope->nph + rope->npw == 64 && rope->row0 >= 0 && (rope->period > 0 ? (rope->row0 + rope->period <= rope->f * rope->h * rope->w && rows % rope->period == 0) : rope->row0 + rows <= rope->f * rope->h * rope->w),
                "rope grid %dx%dx%d does not cover rows [%d, %d)", rope->f, rope->h, rope->w, rope->row0, rope->row0 + rows);
    if (rows <= 0) return SVI_OK;
    dim3 grid_r((rows + ROWS_PER_BLOCK * RPW - 1) / (ROWS_PER_BLOCK * RPW), 2), block(256);
    with_maxc(dim / 8, [&](auto mc) {
        constexpr int MAXC = decltype(mc)::value;
        if constexpr (MAXC <= 10) hipLaunchKernelGGL((rmsnorm_rope_rows_kernel<MAXC, RPW, true, true>), grid_r, block, 0, st, x, ld, rows, dim, weight, weight1, eps, *rope, out_scale, out_scale1, out);
    });
    SVI_LAUNCH_CHECK();
    return SVI_OK;
}

svi_status svi_launch_rmsnorm_rope(bf16* x, int ld, int rows, int dim, const bf16* weight, float eps,
                                   const SviRope* rope, float out_scale, hipStream_t st) {
    return svi_launch_rmsnorm_rope2(x, ld, rows, dim, weight, nullptr, eps, rope, out_scale, 1.0f, st);
}

// weight1 != nullptr: a second operand at columns [dim, 2 dim) of every row gets weight1 / out_scale1 in the same launch
svi_status svi_launch_rmsnorm_rope2(bf16* x, int ld, int rows, int dim, const bf16* weight, const bf16* weight1, float eps,
                                    const SviRope* rope, float out_scale, float out_scale1, hipStream_t st, const SviScatter* scatter) {
    SVI_REQUIRE(dim % 8 == 0 && ld % 8 == 0, "rmsnorm: dim/ld must be multiples of 8");
    SVI_REQUIRE(dim <= 8192, "rmsnorm: dim %d > 8192 unsupported", dim);
    if (rows <= 0) return SVI_OK;
    SviRope r{};
    if (rope) {
        r = *rope;
        SVI_REQUIRE(dim % 128 == 0 && r.npf + r.nph + r.npw == 64, "rope needs head_dim 128");
        SVI_REQUIRE(r.row0 >= 0 && (r.period > 0 ? (r.row0 + r.period <= r.f * r.h * r.w && rows % r.period == 0) : r.row0 + rows <= r.f * r.h * r.w),
                    "rope grid %dx%dx%d does not cover rows [%d, %d)", r.f, r.h, r.w, r.row0, r.row0 + rows);
    }
    SVI_REQUIRE(!weight1 || ld >= 2 * dim, "rmsnorm: a second operand needs ld >= 2 dim");
    dim3 grid((rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK, weight1 ? 2 : 1), block(256);
    const int nchunk = dim / 8;
    const int use = rope ? 1 : 0;
    SviScatter sc{};
    if (scatter) {
        sc = *scatter;
        SVI_REQUIRE(sc.out0 && (!weight1 || sc.out1) && sc.P > 0 && sc.Dp > 0 && sc.Dg > 0 && sc.P * sc.Dp == dim && sc.Dp % sc.Dg == 0 && sc.Dg % 8 == 0,
                    "rmsnorm: bad send layout (P=%d Dp=%d Dg=%d for dim %d)", sc.P, sc.Dp, sc.Dg, dim);
        SVI_REQUIRE(sc.rows_per_sample == 0 || (sc.rows_per_sample > 0 && rows % sc.rows_per_sample == 0),
                    "rmsnorm: %d rows are not whole samples of %d rows", rows, sc.rows_per_sample);
    }
    // the DiT's shapes (in place, whole chunks per lane, per-token RoPE table or no RoPE): the multi-row kernel
    const bool multi_row = !scatter && (nchunk == 64 * 3 || nchunk == 64 * 10) && (!rope || r.tab_tok) && svi_switches().rms_rows;
    const dim3 grid_r((rows + ROWS_PER_BLOCK * RPW - 1) / (ROWS_PER_BLOCK * RPW), weight1 ? 2 : 1);
    with_maxc(nchunk, [&](auto mc) {
        constexpr int MAXC = decltype(mc)::value;
        if constexpr (MAXC <= 10) {
            if (multi_row && rope) { hipLaunchKernelGGL((rmsnorm_rope_rows_kernel<MAXC, RPW, true>), grid_r, block, 0, st, x, ld, rows, dim, weight, weight1, eps, r, out_scale, out_scale1); return; }
            if (multi_row) { hipLaunchKernelGGL((rmsnorm_rope_rows_kernel<MAXC, RPW, false>), grid_r, block, 0, st, x, ld, rows, dim, weight, weight1, eps, r, out_scale, out_scale1); return; }
        }
        if (scatter) hipLaunchKernelGGL((rmsnorm_rope_kernel<MAXC, true>), grid, block, 0, st, x, ld, rows, dim, weight, weight1, eps, use, r, out_scale, out_scale1, sc);
        else hipLaunchKernelGGL((rmsnorm_rope_kernel<MAXC, false>), grid, block, 0, st, x, ld, rows, dim, weight, weight1, eps, use, r, out_scale, out_scale1, sc);
    });
    SVI_LAUNCH_CHECK();
    return SVI_OK;
}

// ------------------------------------------------------------------------------------------------
// bf16 transpose through LDS (64x64 tiles): out[c][r] = in[r][c].  Used by the flash_attention seam
// to present V as V^T (the DiT forward never needs it: its V^T comes straight out of a swapped GEMM).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void transpose_kernel(const bf16* __restrict__ in, int ldi, bf16* __restrict__ out,
                                                        int ldo, int rows, int cols) {
    __shared__ bf16 tile[64][66];
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < 64; i += 4) {
        const int r = r0 + i, c = c0 + tx;
        tile[i][tx] = (r < rows && c < cols) ? in[(size_t)r * ldi + c] : (bf16)0.f;
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        const int c = c0 + i, r = r0 + tx;
        if (c < cols && r < rows) out[(size_t)c * ldo + r] = tile[tx][i];
    }
}

svi_status svi_launch_transpose(const bf16* in, int ldi, bf16* out, int ldo, int rows, int cols, hipStream_t st) {
    if (rows <= 0 || cols <= 0) return SVI_OK;
    dim3 grid((cols + 63) / 64, (rows + 63) / 64), block(256);
    hipLaunchKernelGGL(transpose_kernel, grid, block, 0, st, in, ldi, out, ldo, rows, cols);
    SVI_LAUNCH_CHECK();
    return SVI_OK;
}

// ------------------------------------------------------------------------------------------------
// CFG combine + flow-match Euler step (pipelines/svi_video.py:410,420; schedulers/flow_match.py:63)
//   v   = uncond + s*(cond-uncond)        (bf16 tensor ops: each result rounded)
//   lat = lat + v*(sigma_next - sigma)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cfg_step_kernel(bf16* __restrict__ lat, const bf16* __restrict__ cond,
                                                       const bf16* __restrict__ uncond, int64_t n, float s,
                                                       float dsigma) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float c = (float)cond[i];
        float v = c;
        if (uncond) {
            const float u = (float)uncond[i];
            v = rbf(u + rbf(s * rbf(c - u)));
        }
        lat[i] = (bf16)((float)lat[i] + rbf(v * dsigma));
    }
}

svi_status svi_launch_cfg_step(bf16* lat, const bf16* cond, const bf16* uncond, int64_t n, float s, float dsigma,
                               hipStream_t st) {
    if (n <= 0) return SVI_OK;
    hipLaunchKernelGGL(cfg_step_kernel, grid_1d(n, 2048), dim3(256), 0, st, lat, cond, uncond, n, s, dsigma);
    SVI_LAUNCH_CHECK();
    return SVI_OK;
}

__global__ __launch_bounds__(256) void add_bf16_kernel(bf16* __restrict__ a, const bf16* __restrict__ b, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        a[i] = (bf16)((float)a[i] + (float)b[i]);
}

// out = bf16(a - b): the TeaCache residual, hidden_states - previous_hidden_states (pipelines/svi_video.py:65)
__global__ __launch_bounds__(256) void sub_bf16_kernel(bf16* __restrict__ out, const bf16* __restrict__ a, const bf16* __restrict__ b, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        out[i] = (bf16)((float)a[i] - (float)b[i]);
}

svi_status svi_launch_sub_bf16(bf16* out, const bf16* a, const bf16* b, int64_t n, hipStream_t st) {
    if (n <= 0) return SVI_OK;
    hipLaunchKernelGGL(sub_bf16_kernel, grid_1d(n, 4096), dim3(256), 0, st, out, a, b, n);
    SVI_LAUNCH_CHECK();
    return SVI_OK;
}

// out = bf16(a - bf16(b + c)): the TeaCache residual of a branch whose x_before_blocks is the patch embedding b plus add_condition c — add_bf16_kernel's
// rounding point, then sub_bf16_kernel's — without keeping the sum in a buffer (svi_dit_forward_talk3_tea)
__global__ __launch_bounds__(256) void sub_sum_bf16_kernel(bf16* __restrict__ out, const bf16* __restrict__ a, const bf16* __restrict__ b,
                                                           const bf16* __restrict__ c, int64_t n8) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
        const bf16x8 av = ld_bf16x8(a + i * 8), bv = ld_bf16x8(b + i * 8), cv = ld_bf16x8(c + i * 8);
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (bf16)((float)av[j] - (float)(bf16)((float)bv[j] + (float)cv[j]));
        st_bf16x8(out + i * 8, o);
    }
}

// n must be a multiple of 8 and the operands 16-byte aligned (rows of the model width)
svi_status svi_launch_sub_sum_bf16(bf16* out, const bf16* a, const bf16* b, const bf16* c, int64_t n, hipStream_t st) {
    SVI_REQUIRE(out && a && b && c, "sub_sum: null operand");
    SVI_REQUIRE(n % 8 == 0 && (((uintptr_t)out | (uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0, "sub_sum: operands must be 16-byte aligned, n a multiple of 8");
    if (n <= 0) return SVI_OK;
    const int64_t n8 = n / 8;
    hipLaunchKernelGGL(sub_sum_bf16_kernel, grid_1d(n8, 2048), dim3(256), 0, st, out, a, b, c, n8);
    SVI_LAUNCH_CHECK();
    return SVI_OK;
}

svi_status svi_launch_add_bf16(bf16* a, const bf16* b, int64_t n, hipStream_t st) {
    if (n <= 0) return SVI_OK;
    hipLaunchKernelGGL(add_bf16_kernel, grid_1d(n, 4096), dim3(256), 0, st, a, b, n);
    SVI_LAUNCH_CHECK();
    return SVI_OK;
}

// ------------------------------------------------------------------------------------------------
// TeaCache skip step (pipelines/svi_video.py:68-70, then the head's norm, models/wan_video_dit.py:401-404): the branches of a guidance step see the same
// patch-embedded row of X and differ in their cached residual — and, in the talk variant (svi_video_talk.py:448-466), in whether add_condition was added
// to X first: cond and drop-text have it, uncond has not.  One wave reads the row of X once, the add_condition row once where a served branch has one,
// and per served branch its residual row; it forms bf16(x_k + residual_k) — add_bf16_kernel's rounding point, as for x + add_condition — and writes that
// branch's LayerNorm + modulate row through the row body above: each output row has the bits of add_bf16 (+ add_bf16) followed by svi_launch_ln_mod.
// X is left as it is; the add_bf16 pass over X and the LayerNorm launch per branch are gone (a CFG pair: three row reads and two row writes, not six and
// four).  A branch with res[k] == nullptr is not served.  NBR: 2 (a CFG pair) or 3 (the talk variant's cond, uncond, drop-text); ADDC: an add_condition
// row is read (without it the x + add_condition registers do not exist).
// ------------------------------------------------------------------------------------------------
struct SviSkipRows {
    const bf16* res[3];          // the residual rows of a served branch, nullptr otherwise
    bf16* out[3];                // that branch's LayerNorm + modulate rows
    int addc[3];                 // the branch's embedded input has add_condition added
};
template <int MAXC, int NBR, bool ADDC>
__global__ __launch_bounds__(256) void add_ln_mod_skip_kernel(const bf16* __restrict__ x, const bf16* __restrict__ addc, SviSkipRows p, int rows, int dim,
                                                              float eps, const float* __restrict__ shift, const float* __restrict__ scale1p) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nchunk = dim >> 3;
    const size_t roff = (size_t)row * dim;
    bf16x8 xv[MAXC], xa[ADDC ? MAXC : 1];          // the row of X, and bf16(x + add_condition)
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const int ci = lane + 64 * c;
        if (ci < nchunk) {
            xv[c] = ld_bf16x8(x + roff + ci * 8);
            if constexpr (ADDC) {
                const bf16x8 a = ld_bf16x8(addc + roff + ci * 8);
#pragma unroll
                for (int j = 0; j < 8; ++j) xa[c][j] = (bf16)((float)xv[c][j] + (float)a[j]);
            }
        }
    }
#pragma unroll
    for (int br = 0; br < NBR; ++br) {
        const bf16* res = p.res[br];
        if (!res) continue;                              // uniform over the grid
        float v[MAXC][8];
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            const int ci = lane + 64 * c;
            if (ci < nchunk) {
                const bf16x8 r = ld_bf16x8(res + roff + ci * 8);
                bf16x8 xin = xv[c];
                if constexpr (ADDC) { if (p.addc[br]) xin = xa[c]; }
#pragma unroll
                for (int j = 0; j < 8; ++j) v[c][j] = (float)(bf16)((float)xin[j] + (float)r[j]);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[c][j] = 0.f;
            }
        }
        float mean, rstd;
        ln_row_stats<MAXC, false>(v, lane, nchunk, dim, eps, mean, rstd);
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            const int ci = lane + 64 * c;
            if (ci < nchunk) st_bf16x8(p.out[br] + roff + ci * 8, ln_emit_chunk(v[c], mean, rstd, false, true, ln_load_vecs(false, true, nullptr, nullptr, shift, scale1p, ci * 8)));
        }
    }
}

// p.addc[k] may be set only where add_condition is given; at least one branch is served
static svi_status launch_add_ln_mod_skip(const bf16* x, const bf16* add_condition, const SviSkipRows& p, int nbr, int rows, int dim, float eps,
                                         const float* shift, const float* scale1p, hipStream_t st) {
    dim3 grid((rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK), block(256);
    with_maxc(dim / 8, [&](auto mc) {
        constexpr int MAXC = decltype(mc)::value;
        if (nbr == 2) hipLaunchKernelGGL((add_ln_mod_skip_kernel<MAXC, 2, false>), grid, block, 0, st, x, add_condition, p, rows, dim, eps, shift, scale1p);
        else if (add_condition) hipLaunchKernelGGL((add_ln_mod_skip_kernel<MAXC, 3, true>), grid, block, 0, st, x, add_condition, p, rows, dim, eps, shift, scale1p);
        else hipLaunchKernelGGL((add_ln_mod_skip_kernel<MAXC, 3, false>), grid, block, 0, st, x, add_condition, p, rows, dim, eps, shift, scale1p);
    });
    SVI_LAUNCH_CHECK();
    return SVI_OK;
}

// The CFG pair.  x, res_*, out_*: dense [rows, dim] bf16, 16-byte aligned; out_a / out_b are written, x and the residuals only read.
// res_b / out_b may be null: one branch only.
svi_status svi_launch_add_ln_mod_pair(const bf16* x, const bf16* res_a, const bf16* res_b, bf16* out_a, bf16* out_b, int rows, int dim, float eps,
                                      const float* shift, const float* scale1p, hipStream_t st) {
    SVI_REQUIRE(x && res_a && out_a && shift && scale1p && (res_b == nullptr) == (out_b == nullptr), "add + layernorm: null operand");
    SVI_REQUIRE(dim % 8 == 0 && dim <= 8192, "add + layernorm: dim %d must be a multiple of 8, at most 8192", dim);
    SVI_REQUIRE((((uintptr_t)x | (uintptr_t)res_a | (uintptr_t)res_b | (uintptr_t)out_a | (uintptr_t)out_b | (uintptr_t)shift | (uintptr_t)scale1p) & 15) == 0,
                "add + layernorm: operands must be 16-byte aligned");
    if (rows <= 0) return SVI_OK;
    const SviSkipRows p{{res_a, res_b, nullptr}, {out_a, out_b, nullptr}, {0, 0, 0}};
    return launch_add_ln_mod_skip(x, nullptr, p, 2, rows, dim, eps, shift, scale1p, st);
}

// The talk variant.  x, add_condition (may be null), res[k], out[k]: dense [rows, dim] bf16, 16-byte aligned.  Branch k (0 cond, 1 uncond, 2 drop-text) is
// served when res[k] is given; with_addc[k] says whether its input is bf16(x + add_condition) (ignored without add_condition).  Only the out[k] are written.
svi_status svi_launch_add_ln_mod_talk3(const bf16* x, const bf16* add_condition, const bf16* const res[3], bf16* const out[3], const bool with_addc[3],
                                       int rows, int dim, float eps, const float* shift, const float* scale1p, hipStream_t st) {
    SVI_REQUIRE(x && shift && scale1p, "add + layernorm (talk): null operand");
    SVI_REQUIRE(dim % 8 == 0 && dim <= 8192, "add + layernorm (talk): dim %d must be a multiple of 8, at most 8192", dim);
    SviSkipRows p{};
    uintptr_t bits = (uintptr_t)x | (uintptr_t)add_condition | (uintptr_t)shift | (uintptr_t)scale1p;
    bool any = false, any_addc = false;
    for (int k = 0; k < 3; ++k) {
        if (!res[k]) continue;
        SVI_REQUIRE(out[k], "add + layernorm (talk): branch %d has a residual and no output rows", k);
        p.res[k] = res[k]; p.out[k] = out[k]; p.addc[k] = (add_condition && with_addc[k]) ? 1 : 0;
        bits |= (uintptr_t)res[k] | (uintptr_t)out[k];
        any = true;
        any_addc = any_addc || p.addc[k];
    }
    SVI_REQUIRE((bits & 15) == 0, "add + layernorm (talk): operands must be 16-byte aligned");
    if (rows <= 0 || !any) return SVI_OK;
    return launch_add_ln_mod_skip(x, any_addc ? add_condition : nullptr, p, 3, rows, dim, eps, shift, scale1p, st);          // not read when no served branch has it
}


// ------------------------------------------------------------------------------------------------
// Frame hand-off of the clip loop, on the device.  The reference turns the decoded video into 8-bit frames
// (SVIVideoPipeline.tensor2video, pipelines/svi_video.py:366-370: ((x + 1) * 127.5).clip(0, 255).astype(uint8), 'C T H W -> T H W C')
// and turns the last frames back into [-1, 1] floats for the next clip's conditioning (BasePipeline.preprocess_image,
// pipelines/base.py:44-45: float32(x) * (2 / 255) - 1, 'H W C -> C H W').  Same fp32 arithmetic here, so the 8-bit frames and the
// conditioning input are bit-identical to the host round trip — without leaving HBM.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void video_to_u8_kernel(const float* __restrict__ v, unsigned char* __restrict__ out, long thw) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;           // over T*H*W*3 outputs
    if (idx >= thw * 3) return;
    const long px = idx / 3;
    const int c = (int)(idx - px * 3);
    float y = (v[(long)c * thw + px] + 1.0f) * 127.5f;
    y = fminf(fmaxf(y, 0.0f), 255.0f);
    out[idx] = (unsigned char)(int)y;                                       // astype(uint8): truncation
}
__global__ __launch_bounds__(256) void u8_to_video_kernel(const unsigned char* __restrict__ f, float* __restrict__ out, int n, long hw) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;           // over n*3*H*W outputs, [n, 3, H, W]
    if (idx >= (long)n * 3 * hw) return;
    const long px = idx % hw;
    const int c = (int)((idx / hw) % 3);
    const long i = idx / (3 * hw);
    out[idx] = (float)f[(i * hw + px) * 3 + c] * (float)(2.0 / 255.0) - 1.0f;
}

svi_status svi_launch_video_to_u8(const float* video, unsigned char* out, long thw, hipStream_t st) {
    if (thw <= 0) return SVI_OK;
    hipLaunchKernelGGL(video_to_u8_kernel, dim3((unsigned)((thw * 3 + 255) / 256)), dim3(256), 0, st, video, out, thw);
    SVI_LAUNCH_CHECK();
    return SVI_OK;
}
svi_status svi_launch_u8_to_video(const unsigned char* frames, float* out, int n, long hw, hipStream_t st) {
    if (n <= 0 || hw <= 0) return SVI_OK;
    hipLaunchKernelGGL(u8_to_video_kernel, dim3((unsigned)(((long)n * 3 * hw + 255) / 256)), dim3(256), 0, st, frames, out, n, hw);
    SVI_LAUNCH_CHECK();
    return SVI_OK;
}


// ------------------------------------------------------------------------------------------------
// FP8 weight storage (BASELINE configs[4]).  The reference's "FP8 quantization" (test_svi.py:337,
// vram_management/layers.py:65-71) stores every parameter as float8_e4m3fn and casts it to the computation dtype (bf16) in front of
// every use: W_eff = bf16(e4m3(W)) — arithmetic stays bf16.  e4m3fn -> bf16 is exact (3 mantissa bits, exponents 2^-9 .. 2^8), so
// the cast is done ONCE at bind time: 288 GB of HBM hold the bf16 copy next to the fp8 original, and every forward is then the
// ordinary bf16 forward on exactly the reference's effective weights.
// OCP e4m3fn: 1-4-3, bias 7, no infinities, S.1111.111 = NaN, subnormals m * 2^-9.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fp8_e4m3_to_bf16_kernel(const unsigned char* __restrict__ in, bf16* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned b = in[i];
    const unsigned sign = (b & 0x80u) << 24, e = (b >> 3) & 15u, m = b & 7u;
    unsigned bits;
    if (e == 15u && m == 7u) bits = sign | 0x7fc00000u;                                  // NaN
    else if (e == 0u) bits = sign | __builtin_bit_cast(unsigned, (float)m * 0.001953125f);   // subnormal: m * 2^-9 (exact in fp32)
    else bits = sign | ((e + 120u) << 23) | (m << 20);
    out[i] = (bf16)__builtin_bit_cast(float, bits);                                      // exact: the low 16 bits are zero
}
svi_status svi_launch_fp8_e4m3_to_bf16(const unsigned char* in, bf16* out, int64_t n, hipStream_t st) {
    if (n <= 0) return SVI_OK;
    hipLaunchKernelGGL(fp8_e4m3_to_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, in, out, n);
    SVI_LAUNCH_CHECK();
    return SVI_OK;
}


// ------------------------------------------------------------------------------------------------
// Sequence-parallel exchanges, receive side (svi_hip/sequence_parallel.py).  The send side needs no kernel: q | k leave the
// RMSNorm+RoPE launch in send order (SviScatter), V^T [D, ldvt] and the attention output [G][L][Dg] already are contiguous per peer.
// ------------------------------------------------------------------------------------------------
// V^T pieces [P(src)][Dp][lds] -> out.  A piece's columns are the source's token rows, branch b (of nb stacked CFG branches) at columns
// [b * Ls, (b + 1) * Ls) (columns past nb * Ls are padding); channel c = g * Dg + cg of the piece goes to row (g * nb + b) * Dg + cg of out
// [G * nb * Dg][L8], column src * Ls + i: per head group the branches' channels are adjacent — 2 x as many heads of one attention launch.
// nb = 1: out [Dp][L8], row c.  VEC elements per thread.
template <int VEC>
__global__ __launch_bounds__(256) void sp_unpack_vt_kernel(const bf16* __restrict__ recv, bf16* __restrict__ out, int P, int Dp, int Ls, int lds, int L8, int nb, int Dg) {
    const int per_row = Ls / VEC;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = (int64_t)P * Dp * nb * per_row;
    if (idx >= n) return;
    const int i = (int)(idx % per_row) * VEC;
    int64_t rc = idx / per_row;
    const int b = (int)(rc % nb); rc /= nb;
    const int c = (int)(rc % Dp), src = (int)(rc / Dp);
    const int g = c / Dg, cg = c - g * Dg;
    const bf16* ip = recv + ((size_t)src * Dp + c) * lds + (size_t)b * Ls + i;
    bf16* op = out + ((size_t)(g * nb + b) * Dg + cg) * L8 + (size_t)src * Ls + i;
    if constexpr (VEC == 8) st_bf16x8(op, ld_bf16x8(ip));
    else if constexpr (VEC == 2) *reinterpret_cast<unsigned*>(op) = *reinterpret_cast<const unsigned*>(ip);
    else *op = *ip;
}
svi_status svi_launch_sp_unpack_vt(const bf16* recv, bf16* out, int P, int Dp, int Ls, int lds, int L8, hipStream_t st, int nb, int Dg) {
    if (Dg <= 0) Dg = Dp;
    SVI_REQUIRE(P > 0 && Dp > 0 && Ls > 0 && nb >= 1 && lds >= nb * Ls && L8 >= P * Ls && Dp % Dg == 0, "sp_unpack_vt: bad sizes");
    const int vec = (Ls % 8 == 0 && lds % 8 == 0 && L8 % 8 == 0) ? 8 : (Ls % 2 == 0 && lds % 2 == 0 && L8 % 2 == 0) ? 2 : 1;
    const int64_t n = (int64_t)P * Dp * nb * (Ls / vec);
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (vec == 8) hipLaunchKernelGGL(sp_unpack_vt_kernel<8>, grid, block, 0, st, recv, out, P, Dp, Ls, lds, L8, nb, Dg);
    else if (vec == 2) hipLaunchKernelGGL(sp_unpack_vt_kernel<2>, grid, block, 0, st, recv, out, P, Dp, Ls, lds, L8, nb, Dg);
    else hipLaunchKernelGGL(sp_unpack_vt_kernel<1>, grid, block, 0, st, recv, out, P, Dp, Ls, lds, L8, nb, Dg);
    SVI_LAUNCH_CHECK();
    return SVI_OK;
}
// attention output pieces [G][P(src)][Ls][nb][Dg] -> out [nb * Ls][P * G * Dg]: branch b's token rows at [b * Ls, (b + 1) * Ls), source j's head block at
// columns [j*Dp, (j+1)*Dp), Dp = G*Dg
__global__ __launch_bounds__(256) void sp_unpack_out_kernel(const bf16* __restrict__ recv, bf16* __restrict__ out, int P, int G, int Ls, int Dg, int nb) {
    const int cpr = Dg >> 3;                                            // 16-byte chunks per piece row
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n = (int64_t)G * P * Ls * nb * cpr;
    if (idx >= n) return;
    const int ch = (int)(idx % cpr);
    int64_t t = idx / cpr;
    const int b = (int)(t % nb); t /= nb;
    const int row = (int)(t % Ls); t /= Ls;
    const int j = (int)(t % P), g = (int)(t / P);
    const int D = P * G * Dg;
    st_bf16x8(out + ((size_t)b * Ls + row) * D + (size_t)j * G * Dg + (size_t)g * Dg + ch * 8, ld_bf16x8(recv + idx * 8));
}
svi_status svi_launch_sp_unpack_out(const bf16* recv, bf16* out, int P, int G, int Ls, int Dg, hipStream_t st, int nb) {
    SVI_REQUIRE(P > 0 && G > 0 && Ls > 0 && Dg > 0 && Dg % 8 == 0 && nb >= 1, "sp_unpack_out: bad sizes");
    const int64_t n = (int64_t)G * P * Ls * nb * (Dg / 8);
    hipLaunchKernelGGL(sp_unpack_out_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, recv, out, P, G, Ls, Dg, nb);
    SVI_LAUNCH_CHECK();
    return SVI_OK;
}


// ------------------------------------------------------------------------------------------------
// Three-way guidance of the talk sampler + Euler step (pipelines/svi_video_talk.py:455-461, schedulers/flow_match.py:63):
//   v = uncond + s_text * (cond - drop_text) + s_audio * (drop_text - uncond)      (bf16 tensor ops, left to right, each rounded)
//   lat = lat + v * (sigma_next - sigma)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cfg3_step_kernel(bf16* __restrict__ lat, const bf16* __restrict__ cond, const bf16* __restrict__ uncond,
                                                        const bf16* __restrict__ drop, int64_t n, float st, float sa, float dsigma) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float c = (float)cond[i], u = (float)uncond[i], d = (float)drop[i];
        const float a = rbf(st * rbf(c - d));
        const float b = rbf(sa * rbf(d - u));
        const float v = rbf(rbf(u + a) + b);
        lat[i] = (bf16)((float)lat[i] + rbf(v * dsigma));
    }
}
svi_status svi_launch_cfg3_step(bf16* lat, const bf16* cond, const bf16* uncond, const bf16* drop, int64_t n, float st, float sa, float dsigma,
                                hipStream_t stream) {
    if (n <= 0) return SVI_OK;
    hipLaunchKernelGGL(cfg3_step_kernel, grid_1d(n, 2048), dim3(256), 0, stream, lat, cond, uncond, drop, n, st, sa, dsigma);
    SVI_LAUNCH_CHECK();
    return SVI_OK;
}


// ------------------------------------------------------------------------------------------------
// Clip audio windows of the talk stream, cut on the device (SVITalkVideoPipeline.get_audio_embedding + preprocess_audio + .to(bfloat16),
// pipelines/svi_video_talk.py:412-446).  emb [N, R] holds one row per audio frame of the whole stream (R = 12 blocks x 768 channels in the real
// model); a clip that starts at audio frame `start` and has T latent frames (4 (T - 1) + 1 video frames, window 5) reads, for video frame f and window
// position w, row clamp(start + f + (w - 2), 0, N - 1):
//   first  [5, R]         : video frame 0, positions 0..4
//   latter [T - 1, 8, R]  : latent frame t = video frames 1 + 4t .. 4 + 4t: positions 0, 1, 2 of the first, the centre of the two middle ones,
//                           positions 2, 3, 4 of the last
// A clamped gather and one rounding to bf16 (round to nearest even, torch's): the result is defined bit for bit.
// One workgroup = 256 16-byte chunks of ONE output row: the row's source index is worked out once, on the scalar unit (blockIdx only).
// ------------------------------------------------------------------------------------------------
template <typename SRC>
__global__ __launch_bounds__(256) void audio_windows_kernel(const SRC* __restrict__ emb, int N, int R, long start, bf16* __restrict__ first, bf16* __restrict__ latter) {
    const int r = blockIdx.x;                                   // output row: 0..4 = first, 5 + 8 t + j = latter[t][j]
    long f, w;
    bf16* out;
    if (r < 5) { f = 0; w = r; out = first + (size_t)r * R; }
    else {
        const int q = r - 5, t = q >> 3, j = q & 7;
        f = 1 + 4 * (long)t + (j < 3 ? 0 : j == 3 ? 1 : j == 4 ? 2 : 3);
        w = j < 3 ? j : j < 5 ? 2 : j - 3;
        out = latter + (size_t)q * R;
    }
    long src = start + f + w - 2;
    src = src < 0 ? 0 : src > (long)N - 1 ? (long)N - 1 : src;
    const int c = (blockIdx.y * 256 + threadIdx.x) * 8;
    if (c >= R) return;                                         // R % 8 == 0: a chunk is inside the row or past it
    const SRC* ip = emb + (size_t)src * R + c;
    if constexpr (sizeof(SRC) == 2) st_bf16x8(out + c, ld_bf16x8(reinterpret_cast<const bf16*>(ip)));
    else {
        const f32x4 a = *reinterpret_cast<const f32x4*>(ip), b = *reinterpret_cast<const f32x4*>(ip + 4);
        bf16x8 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] = (bf16)a[e]; v[4 + e] = (bf16)b[e]; }
        st_bf16x8(out + c, v);
    }
}
svi_status svi_launch_audio_windows(const void* emb, bool f32, int N, int R, int start, int T, bf16* first, bf16* latter, hipStream_t st) {
    SVI_REQUIRE(emb && first && (T == 1 || latter), "audio windows: null argument");
    SVI_REQUIRE(N >= 1 && T >= 1 && start >= 0 && R > 0 && R % 8 == 0, "audio windows: bad sizes (N %d, R %d, start %d, T %d)", N, R, start, T);
    SVI_REQUIRE(T <= (1 << 24), "audio windows: %d latent frames", T);
    SVI_REQUIRE((((uintptr_t)emb | (uintptr_t)first | (uintptr_t)latter) & 15) == 0, "audio windows: operands must be 16-byte aligned");
    const dim3 grid((unsigned)(5 + 8 * (T - 1)), (unsigned)((R / 8 + 255) / 256)), block(256);
    if (f32) hipLaunchKernelGGL(audio_windows_kernel<float>, grid, block, 0, st, reinterpret_cast<const float*>(emb), N, R, (long)start, first, latter);
    else hipLaunchKernelGGL(audio_windows_kernel<bf16>, grid, block, 0, st, reinterpret_cast<const bf16*>(emb), N, R, (long)start, first, latter);
    SVI_LAUNCH_CHECK();
    return SVI_OK;
}
