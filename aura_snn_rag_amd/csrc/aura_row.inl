// aura_row.inl -- what one wave derives from one fp32 row: the sum of squares behind 1/||row|| and the bf16 shadow row
// with its rounding-error norm.  One definition each, shared by aura_knn.hip (row norms, the write kernels),
// aura_bank.hip (the shadow kernels, the inverted lists' upkeep) and aura_blend.hip (a blended row's derived state), so
// that a row's cached norm, shadow and rho carry the same bits whichever kernel produced them.  Included inside each
// file's anonymous namespace; needs aura_common.inl.  The row may live in global memory or in LDS.
#pragma once

typedef float f32x8b __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8b __attribute__((ext_vector_type(8)));

// sum of squares of p[0 .. D) on every lane: a per-lane fmaf chain (16-byte loads with vec4) and a butterfly
__device__ __forceinline__ float wave_row_sumsq(const float* __restrict__ p, int64_t D, int lane, bool vec4) {
    float s = 0.0f;
    if (vec4) {
        for (int64_t i = lane * 4; i < D; i += 256) {
            const float4 v = *reinterpret_cast<const float4*>(p + i);
            s = fmaf(v.x, v.x, s); s = fmaf(v.y, v.y, s); s = fmaf(v.z, v.z, s); s = fmaf(v.w, v.w, s);
        }
    } else {
        for (int64_t i = lane; i < D; i += 64) s = fmaf(p[i], p[i], s);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    return s;
}

// One wave converts one row: dst[j] = bf16(src[j] * inv) for j < D (D % 8 == 0, 16-byte chunks);
// returns (on every lane) rho = 1.001 * ||bf16(x) - x||_2 + (D/2 + 3) 2^-24, x = fl(src * inv).
// The second term covers fl(src * inv) against src / ||src|| (rounding of the product and of
// inv_norm's own sum / sqrt / division); the factor the rounding of this very reduction.
__device__ __forceinline__ float shadow_convert_row(const float* __restrict__ src, float inv,
                                                    uint16_t* __restrict__ dst, int64_t D, int lane) {
    float e2 = 0.0f;
    for (int64_t c = lane; c < D / 8; c += 64) {
        const float4 u = *reinterpret_cast<const float4*>(src + 8 * c);
        const float4 w = *reinterpret_cast<const float4*>(src + 8 * c + 4);
        f32x8b x;
        x[0] = u.x * inv; x[1] = u.y * inv; x[2] = u.z * inv; x[3] = u.w * inv;
        x[4] = w.x * inv; x[5] = w.y * inv; x[6] = w.z * inv; x[7] = w.w * inv;
        const bf16x8b b = __builtin_convertvector(x, bf16x8b);
        *reinterpret_cast<bf16x8b*>(dst + 8 * c) = b;
        const f32x8b back = __builtin_convertvector(b, f32x8b);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float d = back[e] - x[e];          // exact: both within a factor 2 of each other
            e2 = fmaf(d, d, e2);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) e2 += __shfl_xor(e2, off);
    return aura_rho_from_e2(e2, (float)D);
}

// ---- IEEE half image (the list-sorted image of the inverted lists) ----
// half(x) for |x| <= 1: round to nearest, ties to even; |x| < 2^-14 is stored as +0, so the image holds no
// subnormal and the bound does not depend on how the matrix pipe treats them.  (An x just below 2^-14 that would
// round UP to 2^-14 is flushed too: the rule is on x, the residual is taken against what is stored.)  65504 is
// never reached.  aura_half_flush is the rule on one element; tests/half_image_rule.py is its host model.
typedef _Float16 f16x8b __attribute__((ext_vector_type(8)));
constexpr float aura_half_min_normal = 6.103515625e-05f;      // 2^-14

__device__ __forceinline__ f32x8b aura_half_flush(f32x8b x) {
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = fabsf(x[e]) < aura_half_min_normal ? 0.0f : x[e];
    return x;
}

// shadow_convert_row's twin for the half image: dst[j] = half(src[j] * inv) under the rule above; returns rho16 (the
// formula of aura_rho_from_e2 on the half residual).  rho_bf16 receives what shadow_convert_row returns for the same
// row, bit for bit (same chunks per lane, same fmaf order, same butterfly): the row-ordered shadow's rho stays current
// whichever kernel converted the row last.
__device__ __forceinline__ float shadow_convert_row_f16(const float* __restrict__ src, float inv,
                                                        uint16_t* __restrict__ dst, int64_t D, int lane,
                                                        float& rho_bf16) {
    float e2 = 0.0f, e2b = 0.0f;
    for (int64_t c = lane; c < D / 8; c += 64) {
        const float4 u = *reinterpret_cast<const float4*>(src + 8 * c);
        const float4 w = *reinterpret_cast<const float4*>(src + 8 * c + 4);
        f32x8b x;
        x[0] = u.x * inv; x[1] = u.y * inv; x[2] = u.z * inv; x[3] = u.w * inv;
        x[4] = w.x * inv; x[5] = w.y * inv; x[6] = w.z * inv; x[7] = w.w * inv;
        const f16x8b h = __builtin_convertvector(aura_half_flush(x), f16x8b);
        *reinterpret_cast<f16x8b*>(dst + 8 * c) = h;
        const f32x8b back = __builtin_convertvector(h, f32x8b);
        const f32x8b backb = __builtin_convertvector(__builtin_convertvector(x, bf16x8b), f32x8b);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float d = back[e] - x[e];          // exact: within a factor 2 of each other, or back = 0
            e2 = fmaf(d, d, e2);
            const float db = backb[e] - x[e];
            e2b = fmaf(db, db, e2b);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { e2 += __shfl_xor(e2, off); e2b += __shfl_xor(e2b, off); }
    rho_bf16 = aura_rho_from_e2(e2b, (float)D);
    return aura_rho_from_e2(e2, (float)D);
}
