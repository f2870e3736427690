// svi_fp8.h — OCP e4m3fn <-> fp32 in integer arithmetic, the same on the host and on the device (plain C++, no HIP types), so the
// rounding can be checked against torch's on a CPU.
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SVI_HD __host__ __device__ __forceinline__
#else
#define SVI_HD inline
#endif

SVI_HD uint32_t svi_f32_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
SVI_HD float svi_bits_f32(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// e4m3fn code -> fp32 (exact).  1-4-3, bias 7, no infinities, S.1111.111 = NaN, subnormals m * 2^-9.
SVI_HD float svi_e4m3fn_to_f32(uint32_t b) {
    const uint32_t sign = (b & 0x80u) << 24, e = (b >> 3) & 15u, m = b & 7u;
    if (e == 15u && m == 7u) return svi_bits_f32(sign | 0x7fc00000u);
    if (e == 0u) return svi_bits_f32(sign | svi_f32_bits((float)m * 0.001953125f));
    return svi_bits_f32(sign | ((e + 120u) << 23) | (m << 20));
}

// fp32 -> e4m3fn code with the semantics of torch's `tensor.to(torch.float8_e4m3fn)` (c10::Float8_e4m3fn): round to nearest even on
// the 3-bit mantissa, subnormals down to 2^-9 (2^-10 ties to 0); NO saturation — the largest finite code is 448, 464 is the tie that
// still rounds to it, anything above (480 = the bit pattern of the NaN code, inf, NaN) becomes NaN (0x7f | sign).  The matrix-core
// quantisers (mx8_quant8) clamp to +-448 in front of v_cvt_pk_fp8_f32 instead; that is not this rule.
SVI_HD uint32_t svi_f32_to_e4m3fn(float f) {
    const uint32_t bits = svi_f32_bits(f);
    const uint32_t sign = (bits >> 24) & 0x80u;
    uint32_t a = bits & 0x7fffffffu;
    uint32_t code;
    if (a > 0x43e80000u) {                                   // |f| > 464 (or inf / NaN): rounds to the NaN code
        code = 0x7fu;
    } else if (a < 0x3c800000u) {                            // |f| < 2^-6: subnormal result, a multiple of 2^-9.  Adding 2^14 aligns the
        const float r = svi_bits_f32(a) + 16384.0f;          // binary point there (ulp(2^14) = 2^-9) and the fp32 add rounds to nearest even
        code = svi_f32_bits(r) - 0x46800000u;                // 0 .. 8; 8 = 2^-6, the smallest normal (code 0x08)
    } else {
        const uint32_t odd = (a >> 20) & 1u;
        a += 0xc407ffffu + odd;                              // re-bias the exponent (127 -> 7: -(120 << 23)) and add half an ulp minus one, plus the tie bit
        code = a >> 20;                                      // 464 -> 0x7e (448): its kept mantissa 110 is even
    }
    return code | sign;
}
