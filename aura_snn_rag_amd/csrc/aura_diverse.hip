// aura_diverse.hip -- diverse recall: a greedy maximal-marginal-relevance selection of k rows among the F
// candidates a recall returned, one kernel for gfx950.  [build-side] no upstream counterpart.
//
// The rule (include/aura_hip.h states it in full): candidates j = 0..F-1 in rank order; cos(i, j) is the fp32
// dot product of the two bank rows, each scaled by its inv_norm; S = the picks so far, m(c) = max cos(c, S);
// eligible = valid, unpicked and (S empty or m(c) < tau); value = (1 - d) score[c] - d m(c) (no second term
// while S is empty); the largest value wins, equal values go to the smaller j; k picks at most.
//
// One workgroup of 4 waves per query.  The F candidate rows (padded to FR = a multiple of 32 with zero rows)
// stream once through LDS in chunks of 64 columns, scaled by inv_norm on the way in; the FR x FR Gram matrix
// of the scaled rows is accumulated in registers on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32: exact fp32,
// an fmaf chain per element), 32 x 32 tiles dealt round-robin to the waves (FR = 32 has one tile: its four
// waves split every chunk's columns instead and their partial sums are added when read).  The Gram then takes
// the staging buffer's place in LDS (64 KB at FR = 128) and wave 0 runs the k greedy steps on it: two
// candidates per lane, one wave argmax per step, m(c) updated from the picked candidate's Gram row.
// No atomics, no scratch in HBM; every row id is range-checked before it becomes an address.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/aura_hip.h"
#include "aura_common.inl"

#pragma clang fp contract(off)

namespace {

constexpr int DV_THREADS = 256;
constexpr int DV_BK = 64;               // columns per chunk
constexpr int DV_STRIDE = DV_BK + 4;    // LDS row stride in floats: 16 rows x 16 B cover the 64 banks once
constexpr int DV_MAX_F = 128;
constexpr int64_t DV_MAX_D = 4096;

template <int T>
constexpr int dv_lds_floats() {
    constexpr int FR = 32 * T;
    constexpr int stage = FR * DV_STRIDE;
    constexpr int gram = (T == 1 ? 4 : 1) * FR * FR;
    return stage > gram ? stage : gram;
}

// (eligible, value, j): is a better than b?  Larger value first, equal (or unordered) values -> smaller j.
__device__ __forceinline__ bool dv_better(bool ea, float va, int ja, bool eb, float vb, int jb) {
    if (ea != eb) return ea;
    if (va > vb) return true;
    if (va < vb) return false;
    return ja < jb;
}

template <int T>
__global__ __launch_bounds__(DV_THREADS) void diverse_select_kernel(
    const float* __restrict__ bank, const float* __restrict__ inv_norm, int64_t count, int64_t D,
    const int32_t* __restrict__ cand_rows, const float* __restrict__ cand_scores, int F, int k, float d, float tau,
    float* __restrict__ out_scores, int32_t* __restrict__ out_rows) {
    constexpr int FR = 32 * T;                       // candidates padded to whole tiles
    constexpr int NT = T * T;                        // 32 x 32 tiles of the Gram
    constexpr int KS = T == 1 ? 4 : 1;               // waves sharing one tile split the chunk's columns
    constexpr int TPW = (NT + 3) / 4;                // tiles per wave
    constexpr int NLD = FR * (DV_BK / 4) / DV_THREADS;   // float4 loads per thread and chunk
    extern __shared__ __attribute__((aligned(16))) float smem[];   // [FR][DV_STRIDE] staging, then [KS][FR][FR] Gram
    __shared__ int s_row[DV_MAX_F];
    __shared__ float s_score[DV_MAX_F];
    __shared__ float s_inv[DV_MAX_F];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 31, lh = lane >> 5;
    const int64_t q = blockIdx.x;

    if (tid < FR) {
        int r = -1;
        float sc = -INFINITY, inv = 0.0f;
        if (tid < F) {
            const int rr = cand_rows[q * F + tid];
            sc = cand_scores[q * F + tid];
            if (rr >= 0 && (int64_t)rr < count && sc == sc) {   // the only place a candidate becomes an address
                r = rr;
                inv = inv_norm[rr];
            }
        }
        s_row[tid] = r;
        s_score[tid] = sc;
        s_inv[tid] = inv;
    }
    __syncthreads();

    // ---- Gram of the scaled rows
    const float* src[NLD];
    float scale[NLD];
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int f = tid + i * DV_THREADS;
        const int r = s_row[f >> 4];
        src[i] = r >= 0 ? bank + (int64_t)r * D + (f & 15) * 4 : nullptr;
        scale[i] = s_inv[f >> 4];
    }
    float4 pre[NLD];
    auto gload = [&](int64_t k0) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int f = tid + i * DV_THREADS;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (src[i] && k0 + (f & 15) * 4 < D) {       // D % 4 == 0: the 16 bytes lie inside the row
                v = *reinterpret_cast<const float4*>(src[i] + k0);
                v.x *= scale[i]; v.y *= scale[i]; v.z *= scale[i]; v.w *= scale[i];
            }
            pre[i] = v;
        }
    };
    f32x16 acc[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.0f;

    const int64_t KT = (D + DV_BK - 1) / DV_BK;
    gload(0);
    for (int64_t kt = 0; kt < KT; ++kt) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int f = tid + i * DV_THREADS;
            *reinterpret_cast<float4*>(smem + (f >> 4) * DV_STRIDE + (f & 15) * 4) = pre[i];
        }
        __syncthreads();
        if (kt + 1 < KT) gload((kt + 1) * DV_BK);
        // lane (li, lh) feeds A[i = li][k] and B[k][j = li] with the same 4 columns 8 kk + 4 lh .. + 3 of a step
        if (T == 1) {
            const float* row = smem + li * DV_STRIDE + 4 * lh;
#pragma unroll
            for (int kk = 0; kk < DV_BK / 8 / KS; ++kk) {
                const float4 v = *reinterpret_cast<const float4*>(row + (wave * (DV_BK / 8 / KS) + kk) * 8);
                acc[0] = aura_mfma_f32_x4(v, v, acc[0]);
            }
        } else {
#pragma unroll
            for (int kk = 0; kk < DV_BK / 8; ++kk) {
#pragma unroll
                for (int t = 0; t < TPW; ++t) {
                    const int tile = wave + 4 * t;          // wave-uniform
                    if (tile < NT) {
                        const float4 av = *reinterpret_cast<const float4*>(
                            smem + ((tile / T) * 32 + li) * DV_STRIDE + 4 * lh + kk * 8);
                        const float4 bv = *reinterpret_cast<const float4*>(
                            smem + ((tile % T) * 32 + li) * DV_STRIDE + 4 * lh + kk * 8);
                        acc[t] = aura_mfma_f32_x4(av, bv, acc[t]);
                    }
                }
            }
        }
        __syncthreads();
    }
    // the staging buffer is free (barrier above): accumulator element e of lane (li, lh) is
    // row (e & 3) + 8 (e >> 2) + 4 lh, column li of its tile
    float* gram = smem;
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int tile = T == 1 ? 0 : wave + 4 * t;
        if (tile < NT) {
            float* g = gram + (T == 1 ? wave * FR * FR : 0) + (tile / T) * 32 * FR + (tile % T) * 32 + li;
#pragma unroll
            for (int e = 0; e < 16; ++e) g[((e & 3) + 8 * (e >> 2) + 4 * lh) * FR] = acc[t][e];
        }
    }
    __syncthreads();
    if (wave != 0) return;

    // ---- k greedy steps, wave 0: lane owns candidates lane and lane + 64
    constexpr int CPL = FR > 64 ? 2 : 1;
    bool valid[CPL], picked[CPL];
    float score[CPL], m[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        const int j = lane + 64 * c;
        valid[c] = j < FR && s_row[j < FR ? j : 0] >= 0;
        score[c] = s_score[j < FR ? j : 0];
        picked[c] = false;
        m[c] = 0.0f;
    }
    const float om = 1.0f - d;
    int mine[2] = {-1, -1};                             // pick number lane + 64 i, kept by its output lane
    for (int s = 0; s < k; ++s) {
        bool be = false;
        float bv = 0.0f;
        int bj = 0x7fffffff;
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const bool e = valid[c] && !picked[c] && (s == 0 || m[c] < tau);
            const float v = (s == 0 || !(d > 0.0f)) ? om * score[c] : om * score[c] - d * m[c];
            const int j = lane + 64 * c;
            if (dv_better(e, v, j, be, bv, bj)) { be = e; bv = v; bj = j; }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const bool oe = __shfl_xor((int)be, off) != 0;
            const float ov = __shfl_xor(bv, off);
            const int oj = __shfl_xor(bj, off);
            if (dv_better(oe, ov, oj, be, bv, bj)) { be = oe; bv = ov; bj = oj; }
        }
        be = __shfl((int)be, 0) != 0;
        bj = __shfl(bj, 0);
        if (!be) break;                                 // nobody is eligible: the tail stays padding
        if ((s & 63) == lane) mine[s >> 6] = bj;
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
            const int j = lane + 64 * c;
            if (j == bj) picked[c] = true;
            if (j < FR) {
                float g = gram[bj * FR + j];
#pragma unroll
                for (int p = 1; p < KS; ++p) g += gram[p * FR * FR + bj * FR + j];
                m[c] = s == 0 ? g : fmaxf(m[c], g);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int o = lane + 64 * i;
        if (o < k) {
            const int p = mine[i];
            out_rows[q * k + o] = p >= 0 ? s_row[p] : -1;
            out_scores[q * k + o] = p >= 0 ? s_score[p] : -INFINITY;
        }
    }
}

template <int T>
int launch_diverse(const float* bank, const float* inv_norm, int64_t count, int64_t D, const int32_t* cand_rows,
                   const float* cand_scores, int64_t nq, int F, int k, float d, float tau, float* out_scores,
                   int32_t* out_rows, hipStream_t s) {
    constexpr int lds = dv_lds_floats<T>() * (int)sizeof(float);
    if (lds + 3 * DV_MAX_F * 4 > 64 * 1024) {
        const int rc = aura_ensure_lds_attr(reinterpret_cast<const void*>(&diverse_select_kernel<T>), lds);
        if (rc != AURA_OK) return rc;
    }
    hipLaunchKernelGGL(diverse_select_kernel<T>, dim3((unsigned)nq), dim3(DV_THREADS), lds, s, bank, inv_norm, count, D,
                       cand_rows, cand_scores, F, k, d, tau, out_scores, out_rows);
    return aura_check_launch();
}

}  // namespace

extern "C" {

int64_t aura_diverse_select_workspace_bytes(int64_t nq, int64_t F, int64_t k) {
    if (nq < 0 || nq > 0x7fffffffLL || k < 1 || k > F || F > DV_MAX_F) return -1;
    return 0;                                           // the Gram lives in LDS
}

int aura_diverse_select(const float* bank, const float* inv_norm, int64_t count, int64_t D, const int32_t* cand_rows,
                        const float* cand_scores, int64_t nq, int64_t F, int64_t k, float diversity,
                        float max_similarity, float* out_scores, int32_t* out_rows, void* workspace,
                        int64_t workspace_bytes, void* stream) {
    const int64_t need = aura_diverse_select_workspace_bytes(nq, F, k);
    if (need < 0 || workspace_bytes < need || (need > 0 && !workspace)) return AURA_E_INVAL;
    if (count < 0 || count > 0x7fffffffLL || D < 4 || D % 4 != 0 || D > DV_MAX_D) return AURA_E_INVAL;
    if (!(diversity >= 0.0f && diversity <= 1.0f) || max_similarity != max_similarity) return AURA_E_INVAL;
    if (nq == 0) return AURA_OK;
    if (!bank || !inv_norm || !cand_rows || !cand_scores || !out_scores || !out_rows) return AURA_E_INVAL;
    if (reinterpret_cast<uintptr_t>(bank) & 15) return AURA_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int f = (int)F, kk = (int)k;
    switch ((f + 31) / 32) {
    case 1: return launch_diverse<1>(bank, inv_norm, count, D, cand_rows, cand_scores, nq, f, kk, diversity,
                                     max_similarity, out_scores, out_rows, s);
    case 2: return launch_diverse<2>(bank, inv_norm, count, D, cand_rows, cand_scores, nq, f, kk, diversity,
                                     max_similarity, out_scores, out_rows, s);
    case 3: return launch_diverse<3>(bank, inv_norm, count, D, cand_rows, cand_scores, nq, f, kk, diversity,
                                     max_similarity, out_scores, out_rows, s);
    default: return launch_diverse<4>(bank, inv_norm, count, D, cand_rows, cand_scores, nq, f, kk, diversity,
                                      max_similarity, out_scores, out_rows, s);
    }
}

}  // extern "C"
