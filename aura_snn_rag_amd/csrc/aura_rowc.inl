// aura_rowc.inl -- per-row score constants of the two-stage recall, shared by aura_knn.hip (prep kernels,
// the cached constants of the inverted lists) and aura_bank.hip (aura_ivf2_append keeps a cached table
// current).  See aura_knn_coarse.inl's header for the bound these constants implement.  Needs aura_common.inl.
#pragma once

// E_fix = 2 D 2^-24 + 1e-5: fp32 accumulation of D terms in either pipe + association of the score formulas
__host__ __device__ __forceinline__ float aura_e_fix(float D) { return 2.0f * D * 5.9604645e-8f + 1e-5f; }

// EQ_WORST bounds the query part of the error for any query (round-to-nearest: ||e_q|| <= 2^-8 ||q_hat||)
__host__ __device__ __forceinline__ float coarse_eq_worst(float D) {
    return (1.001f * 0.00390625f * 1.00001f + (0.5f * D + 3.0f) * 5.9604645e-8f) * 1.0078125f;
}

// The same for the IEEE half image with its subnormal rule (aura_row.inl).  An element that stays normal carries a
// relative error <= 2^-11 (round-to-nearest, 11 significand bits): together at most 2^-11 ||q_hat||.  An element
// below 2^-14 is stored as 0: its error is itself, < 2^-14, and D of them together stay below sqrt(D) 2^-14.  By the
// triangle inequality ||e_q|| <= 2^-11 ||q_hat|| + sqrt(D) 2^-14 with ||q_hat|| <= 1.00001, then the factors of
// aura_rho_from_e2 / aura_eq_from_e2.  (0.0022 at D = 768, below the bf16 constant for every D <= 768; the factor
// 1 + 2^-7 still covers 1 + rho16_row, which obeys the same bound.)
__host__ __device__ __forceinline__ float coarse_eq_worst_f16(float D) {
    return (1.001f * (0.00048828125f * 1.00001f + sqrtf(D) * 6.103515625e-05f) + (0.5f * D + 3.0f) * 5.9604645e-8f) * 1.0078125f;
}

// Per-row score constants {A, B_up, B_lo, w} of the two-stage path (w: centroid id / bank row id).
//   rho != NULL (normalised bf16 shadow rows): A = 0.5 strength, the row's error part from rho[row];
//   rho == NULL (fp32 rows rounded on the fly): A = 0.5 strength / ||row||, worst-case error e_worst.
__device__ __forceinline__ float4 coarse_row_constants(const float4 m, float inv_norm_row, const float* rho_row,
                                                       float now, float e_fix, float e_worst, float eq_worst,
                                                       float w) {
    const float strength = m.x;
    const float tw = aura_time_weight(now, m.y);
    float A, err;
    if (rho_row) {
        A = 0.5f * strength;
        err = 0.5f * fabsf(strength) * (*rho_row + e_fix);
        if (strength < 0.0f) err += fabsf(strength) * eq_worst;     // 2 |A| eq_worst
    } else {
        A = 0.5f * inv_norm_row * strength;
        err = 0.5f * e_worst * fabsf(strength);
    }
    return make_float4(A, tw * strength + err, tw * strength - err, w);
}

// constants of a sorted row of the inverted lists: .w = the bank row id's bits; padding / holes can never
// reach a threshold
__device__ __forceinline__ float4 ivf2_row_constants(int32_t row, const float* __restrict__ meta,
                                                     const float* __restrict__ rho, float now, float D,
                                                     bool f16 = false) {   // f16: rho is rho16, the image IEEE half
    if (row < 0) return make_float4(0.0f, -INFINITY, -INFINITY, __int_as_float(-1));
    const float4 m = *reinterpret_cast<const float4*>(meta + (int64_t)row * 4);
    return coarse_row_constants(m, 0.0f, rho + row, now, aura_e_fix(D), 0.0f,
                                f16 ? coarse_eq_worst_f16(D) : coarse_eq_worst(D), __int_as_float(row));
}
