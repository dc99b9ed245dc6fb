// aura_common.inl -- the pieces every kernel file shares: the launch helpers, the meaning of a tag, the query part of
// the two-stage error bound and the combined score.  One definition each: recall, scoped recall, merging within tags,
// quotas and retention must read a tag and score a row alike to the last bit.  Every .hip file includes it after
// <hip/hip_runtime.h> and include/aura_hip.h; what it defines joins the file's anonymous namespace.  Including it
// switches floating-point contraction off for the rest of the file (the pragma below), as the Makefile's flags do.
#pragma once
#include <mutex>
#include <set>
#include <utility>

#pragma clang fp contract(off)   // the arithmetic below is bit-exact only unfused

namespace {

// ---- host ------------------------------------------------------------------------------------------------------
inline int aura_check_launch() { return hipGetLastError() == hipSuccess ? AURA_OK : AURA_E_LAUNCH; }
inline int64_t aura_align256(int64_t x) { return (x + 255) / 256 * 256; }

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (device, kernel); callable from any host thread and for
// any device of the process.  The state is per translation unit.
inline int aura_ensure_lds_attr(const void* fn, int bytes) {
    static std::mutex mu;
    static std::set<std::pair<int, const void*>> done;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return AURA_E_LAUNCH;
    std::lock_guard<std::mutex> g(mu);
    if (done.count({dev, fn})) return AURA_OK;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return AURA_E_LAUNCH;
    done.insert({dev, fn});
    return AURA_OK;
}

// ---- device ----------------------------------------------------------------------------------------------------
typedef float f32x16 __attribute__((ext_vector_type(16)));   // accumulator of v_mfma_f32_32x32x2_f32

// acc += a b^T over the four k-pairs of one float4 per operand, in k order (exact fp32, a k-ordered fmaf chain)
__device__ __forceinline__ f32x16 aura_mfma_f32_x4(const float4 a, const float4 b, f32x16 acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
    return acc;
}

// The tag of a row from metadata column 3 as stored: an integer in [0, 2^24), else aura_no_tag (negative values, NaN,
// 2^24 and above).  aura_no_tag equals no tag and is not scoped recall's "any tag" (-1) either.
constexpr int aura_no_tag = -2;
__device__ __forceinline__ int aura_row_tag(float w) { return (w > -1.0f && w < 16777216.0f) ? (int)w : aura_no_tag; }

// Rounding-error norm of a normalised row or query rounded to bf16, from its residual e2 = sum (bf16(x) - x)^2:
// rho = 1.001 sqrt(e2) + (D/2 + 3) 2^-24 (aura_bank.hip explains the second term); the query part of the two-stage
// error bound is eq = rho (1 + 2^-7).
__device__ __forceinline__ float aura_rho_from_e2(float e2, float D) {
    return 1.001f * sqrtf(e2) + (0.5f * D + 3.0f) * 5.9604645e-8f;
}
__device__ __forceinline__ float aura_eq_from_e2(float e2, float D) { return aura_rho_from_e2(e2, D) * 1.0078125f; }

// The combined score of a row for a query (hippocampal.py's recall):
//   (0.5 cos + 0.3 / (1 + ||loc_row - loc_q||) + 0.2 exp(-(now - timestamp) / 3600)) * strength
// aura_recency is the bare decay (retention ranks by strength * recency), aura_time_weight the score's third term.
__device__ __forceinline__ float aura_recency(float now, float ts) { return expf(-(now - ts) / 3600.0f); }
__device__ __forceinline__ float aura_time_weight(float now, float ts) { return 0.2f * aura_recency(now, ts); }

// plain form: no locations.  dot = <query, row> unnormalised, iq / inv_m = 1 / their norms, tw = aura_time_weight
__device__ __forceinline__ float aura_score(float dot, float iq, float inv_m, float tw, float strength) {
    return (0.5f * (dot * iq * inv_m) + tw) * strength;
}

// spatial form: with `spatial` set, adds the location term over the first min(sdims, 4) dimensions.  lx: the row's
// location, owned by the caller (a struct of the row's terms returned by value ends up in scratch); q_loc: the
// queries' locations [nq][sdims], read for query q
__device__ __forceinline__ float aura_score_spatial(float dot, float iq, float inv_m, float tw, float strength,
                                                    bool spatial, const float (&lx)[4],
                                                    const float* q_loc, int64_t q, int sdims) {
    float comb = 0.5f * (dot * iq * inv_m);
    if (spatial) {
        float d2 = 0.0f;
        for (int d = 0; d < sdims && d < 4; ++d) {
            const float df = lx[d] - q_loc[q * sdims + d];
            d2 = d2 + df * df;
        }
        comb = comb + 0.3f * (1.0f / (1.0f + sqrtf(d2)));
    }
    return (comb + tw) * strength;
}

}  // namespace
