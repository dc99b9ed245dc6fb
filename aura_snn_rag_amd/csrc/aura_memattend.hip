// aura_memattend.hip -- the cross-attention memory injection of a decoding step over memories that are pinned for the
// generation, folded to two tables per row, in one launch (gfx950).
// The rule is stated once, in include/aura_hip.h ("Memory attend"); the comments here are about how it is computed.
//   One workgroup of eight waves per row.  Every wave loads the whole row (D <= 2048: eight 16-byte units per lane),
//   computes the row's two LayerNorm sums itself and keeps the normalised row in registers: the eight waves hold the
//   same bits and nothing of the prologue crosses a wave.
//   Phase 1.  The H M score rows of G go round the waves in groups of MA_JB consecutive rows; a wave streams its group
//   with 16-byte loads (MA_JB independent loads per unit and lane, addresses clamped instead of branched around),
//   chains the fmaf over its units in ascending order, adds the 64 lane values in the xor butterfly and lane 0 leaves
//   fl(dot + s0) in LDS.  After a barrier one thread per head runs the softmax over its M scores in place.
//   Phase 2.  After a second barrier thread u owns the 16-byte unit u of the output row (D / 4 <= 512 units) and walks
//   the H M rows of U in ascending order: the loads are independent and coalesced, the adds are the rule's chain.
//   The weights come from LDS as broadcast reads.  The thread then adds the bias and the residual and stores its unit.
// Workgroups are independent and nothing depends on R: no atomics, no flags, one pass.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/aura_hip.h"
#include "aura_common.inl"

namespace {

constexpr int MA_WAVES = 8;
constexpr int MA_THREADS = 64 * MA_WAVES;
constexpr int MA_MAX_D = AURA_MEMORY_ATTEND_MAX_D;
constexpr int MA_UNITS = MA_MAX_D / 256;                // float4 units of a row per lane, at most
constexpr int MA_MAX_HM = AURA_MEMORY_ATTEND_MAX_HM;
constexpr int MA_JB = 4;                                // score rows a wave streams together
constexpr int MA_UB = 16;                               // rows of U a thread has in flight

static_assert(MA_MAX_D / 4 <= MA_THREADS, "phase 2 gives every 16-byte unit of the row a thread");

struct MemAttendArgs {
    const float* x;                     // [R][D]
    const float* gamma;                 // [D]
    const float* beta;                  // [D]
    const float* G;                     // [R][H][M][D]
    const float* s0;                    // [R][H][M]
    const float* U;                     // [R][H][M][D]
    const float* bo;                    // [D] or NULL
    float* y;                           // [R][D]
    int D, H, M;
    float eps;
};

__device__ __forceinline__ float ma_wave_sum(float s) {
    s = s + __shfl_xor(s, 32);
    s = s + __shfl_xor(s, 16);
    s = s + __shfl_xor(s, 8);
    s = s + __shfl_xor(s, 4);
    s = s + __shfl_xor(s, 2);
    s = s + __shfl_xor(s, 1);
    return s;
}

__global__ __launch_bounds__(MA_THREADS) void memory_attend_kernel(const MemAttendArgs a) {
    __shared__ float sc[MA_MAX_HM];                                     // the scores, then the weights p
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x;
    const int D = a.D, U4 = D / 4, HM = a.H * a.M;
    const float4* const x4 = reinterpret_cast<const float4*>(a.x) + (int64_t)r * U4;

    // the row, normalised, in registers: lane l holds the units l, l + 64, ..; a unit past the row is zeros
    float4 xh[MA_UNITS];
    {
        const float4* const g4 = reinterpret_cast<const float4*>(a.gamma);
        const float4* const b4 = reinterpret_cast<const float4*>(a.beta);
        float4 gm[MA_UNITS], bt[MA_UNITS];
#pragma unroll
        for (int i = 0; i < MA_UNITS; ++i) {
            if (64 * i < U4) {                                          // wave-uniform
                const int u = lane + 64 * i;
                const int uc = u < U4 ? u : U4 - 1;
                xh[i] = x4[uc];
                gm[i] = g4[uc];
                bt[i] = b4[uc];
            }
        }
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < MA_UNITS; ++i) {
            if (64 * i < U4) {
                const bool live = lane + 64 * i < U4;
                s = s + (live ? xh[i].x : 0.0f);
                s = s + (live ? xh[i].y : 0.0f);
                s = s + (live ? xh[i].z : 0.0f);
                s = s + (live ? xh[i].w : 0.0f);
            }
        }
        const float mu = ma_wave_sum(s) / (float)D;
        float q = 0.0f;
#pragma unroll
        for (int i = 0; i < MA_UNITS; ++i) {
            if (64 * i < U4) {
                const bool live = lane + 64 * i < U4;
                const float dx = live ? xh[i].x - mu : 0.0f, dy = live ? xh[i].y - mu : 0.0f;
                const float dz = live ? xh[i].z - mu : 0.0f, dw = live ? xh[i].w - mu : 0.0f;
                q = q + dx * dx;
                q = q + dy * dy;
                q = q + dz * dz;
                q = q + dw * dw;
            }
        }
        const float var = ma_wave_sum(q) / (float)D;
        const float rstd = 1.0f / sqrtf(var + a.eps);
#pragma unroll
        for (int i = 0; i < MA_UNITS; ++i) {
            if (64 * i < U4) {
                const bool live = lane + 64 * i < U4;
                float4 v;
                v.x = ((xh[i].x - mu) * rstd) * gm[i].x + bt[i].x;
                v.y = ((xh[i].y - mu) * rstd) * gm[i].y + bt[i].y;
                v.z = ((xh[i].z - mu) * rstd) * gm[i].z + bt[i].z;
                v.w = ((xh[i].w - mu) * rstd) * gm[i].w + bt[i].w;
                xh[i] = live ? v : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        }
    }

    // phase 1: the scores
    const float4* const G4 = reinterpret_cast<const float4*>(a.G) + (int64_t)r * HM * U4;
    const float* const s0 = a.s0 + (int64_t)r * HM;
    for (int j0 = wave * MA_JB; j0 < HM; j0 += MA_WAVES * MA_JB) {      // wave-uniform
        const float4* row[MA_JB];
#pragma unroll
        for (int m = 0; m < MA_JB; ++m) row[m] = G4 + (int64_t)(j0 + m < HM ? j0 + m : HM - 1) * U4;
        float t[MA_JB];
#pragma unroll
        for (int m = 0; m < MA_JB; ++m) t[m] = 0.0f;
#pragma unroll
        for (int i = 0; i < MA_UNITS; ++i) {
            if (64 * i < U4) {
                const int u = lane + 64 * i;
                const bool live = u < U4;
                float4 w[MA_JB];
#pragma unroll
                for (int m = 0; m < MA_JB; ++m) w[m] = row[m][live ? u : U4 - 1];
#pragma unroll
                for (int m = 0; m < MA_JB; ++m) {
                    // a lane past the row holds a clamped unit: zero it; its xh is zero too, and fmaf(0, 0, t) == t
                    const float4 wv = live ? w[m] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    float tt = t[m];
                    tt = fmaf(xh[i].x, wv.x, tt);
                    tt = fmaf(xh[i].y, wv.y, tt);
                    tt = fmaf(xh[i].z, wv.z, tt);
                    tt = fmaf(xh[i].w, wv.w, tt);
                    t[m] = tt;
                }
            }
        }
#pragma unroll
        for (int m = 0; m < MA_JB; ++m) {
            const float dot = ma_wave_sum(t[m]);
            if (lane == 0 && j0 + m < HM) sc[j0 + m] = s0[j0 + m] + dot;
        }
    }
    __syncthreads();

    // the softmaxes, one thread per head, in place
    for (int h = threadIdx.x; h < a.H; h += MA_THREADS) {
        float* const p = sc + h * a.M;
        float mx = p[0];
        for (int m = 1; m < a.M; ++m) mx = fmaxf(mx, p[m]);
        float sum = 0.0f;
        for (int m = 0; m < a.M; ++m) {
            const float e = expf(p[m] - mx);
            p[m] = e;
            sum = sum + e;
        }
        for (int m = 0; m < a.M; ++m) p[m] = p[m] / sum;
    }
    __syncthreads();

    // phase 2: the weighted sum of the rows of U, bias and residual
    const int u = threadIdx.x;
    if (u < U4) {
        const float4* const Ucol = reinterpret_cast<const float4*>(a.U) + (int64_t)r * HM * U4 + u;
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        int j = 0;
        for (; j + MA_UB <= HM; j += MA_UB) {
            float4 v[MA_UB];
#pragma unroll
            for (int m = 0; m < MA_UB; ++m) v[m] = Ucol[(int64_t)(j + m) * U4];
#pragma unroll
            for (int m = 0; m < MA_UB; ++m) {
                const float p = sc[j + m];
                acc.x = acc.x + p * v[m].x;
                acc.y = acc.y + p * v[m].y;
                acc.z = acc.z + p * v[m].z;
                acc.w = acc.w + p * v[m].w;
            }
        }
        for (; j < HM; ++j) {
            const float4 v = Ucol[(int64_t)j * U4];
            const float p = sc[j];
            acc.x = acc.x + p * v.x;
            acc.y = acc.y + p * v.y;
            acc.z = acc.z + p * v.z;
            acc.w = acc.w + p * v.w;
        }
        if (a.bo) {
            const float4 b = reinterpret_cast<const float4*>(a.bo)[u];
            acc.x = b.x + acc.x;
            acc.y = b.y + acc.y;
            acc.z = b.z + acc.z;
            acc.w = b.w + acc.w;
        }
        const float4 xv = x4[u];
        float4 out;
        out.x = xv.x + acc.x;
        out.y = xv.y + acc.y;
        out.z = xv.z + acc.z;
        out.w = xv.w + acc.w;
        reinterpret_cast<float4*>(a.y)[(int64_t)r * U4 + u] = out;
    }
}

inline bool misaligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) != 0; }

}  // namespace

extern "C" {

int aura_memory_attend(const float* x, int64_t R, int64_t D, const float* gamma, const float* beta, float eps,
                       const float* G, const float* s0, const float* U, int64_t H, int64_t M,
                       const float* bo_or_null, float* y, void* stream) {
    if (R < 1 || R > AURA_MEMORY_ATTEND_MAX_ROWS || D < 4 || D > MA_MAX_D || D % 4 != 0) return AURA_E_INVAL;
    if (M < 1 || M > AURA_MEMORY_ATTEND_MAX_M || H < 1 || H > MA_MAX_HM || H * M > MA_MAX_HM) return AURA_E_INVAL;
    if (!x || !gamma || !beta || !G || !s0 || !U || !y || !(eps >= 0.0f)) return AURA_E_INVAL;
    if (misaligned(x, 16) || misaligned(gamma, 16) || misaligned(beta, 16) || misaligned(G, 16) || misaligned(U, 16) ||
        misaligned(bo_or_null, 16) || misaligned(y, 16) || misaligned(s0, 4))
        return AURA_E_ALIGN;
    MemAttendArgs a;
    a.x = x; a.gamma = gamma; a.beta = beta;
    a.G = G; a.s0 = s0; a.U = U;
    a.bo = bo_or_null; a.y = y;
    a.D = (int)D; a.H = (int)H; a.M = (int)M;
    a.eps = eps;
    hipLaunchKernelGGL(memory_attend_kernel, dim3((unsigned)R), dim3(MA_THREADS), 0, static_cast<hipStream_t>(stream),
                       a);
    return aura_check_launch();
}

}  // extern "C"
