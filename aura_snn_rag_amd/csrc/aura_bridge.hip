// aura_bridge.hip -- the Poisson bridge of MoELanguageZone: projection, sigmoid, a seeded spike train and its mean over
// the timesteps in one launch (gfx950, wave64).
// The rule is stated once, in include/aura_hip.h ("Poisson bridge"); the comments here are about how it is computed.
//   A workgroup (4 waves) owns 32 consecutive rows and 128 consecutive channels: the rows are staged in LDS as the row
//   operand of v_mfma_f32_32x32x2_f32 (aura_moe.hip's expert linear), the weights come from global memory as the column
//   operand, 16 bytes per lane along k, and a wave owns one block of 32 channels.  The epilogue runs on the accumulator
//   registers: lane (half, l31) holds channel c = block + l31 of the 16 rows (r & 3) + 8 (r >> 2) + 4 half.  Per
//   element: bias, sigmoid, then ceil(T / 4) Philox4x32-10 evaluations whose four words are four timesteps, the
//   comparisons and the count.  Neither the uniforms nor the spike train leave the registers unless the train is asked
//   for.  A row of the row operand touches no other row's result and the counter of a draw names (channel, word group,
//   position, stream), so a row's bits do not depend on its tile, on N or on the launch.
// No atomics, no scratch, one barrier (after the staging), no host read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/aura_hip.h"
#include "aura_common.inl"

namespace {

constexpr int BR_ROWS = 32;
constexpr int BR_MAX_K = AURA_MOE_MAX_DM;
constexpr int BR_STRIDE_MAX = BR_MAX_K + 4;         // a row of the tile and four floats: rows stay 16-byte aligned

struct BridgeArgs {
    const float *x, *W, *b;
    const uint32_t* streams;
    const int32_t* start_dev;           // [B] or NULL: `start` for every stream
    float *rate, *q, *spikes;
    int64_t N, S;
    int K, H, T;
    uint32_t start, seed_lo, seed_hi;
};

struct Words { uint32_t w[4]; };

// all four words of Philox4x32-10, counter (c0, c1, c2, c3), key (k0, k1): the constants of "Replay"
__device__ __forceinline__ Words bridge_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                               uint32_t k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1;
        c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Words{{c0, c1, c2, c3}};
}

__global__ __launch_bounds__(256) void poisson_rate_kernel(const BridgeArgs a) {
    __shared__ float4 s_x[BR_ROWS * BR_STRIDE_MAX / 4];
    __shared__ uint32_t s_pos[BR_ROWS], s_stream[BR_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int K = a.K, H = a.H, T = a.T, stride = K + 4, qk = K / 4;
    const int64_t row0 = (int64_t)blockIdx.x * BR_ROWS;
    float* const xs = reinterpret_cast<float*>(s_x);
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int i = tid; i < BR_ROWS * qk; i += 256) {
        const int row = i / qk, c = i - row * qk;
        float4 v = zero;
        if (row0 + row < a.N) v = reinterpret_cast<const float4*>(a.x)[(row0 + row) * qk + c];
        *reinterpret_cast<float4*>(xs + row * stride + 4 * c) = v;
    }
    if (tid < BR_ROWS) {
        const int64_t n = row0 + tid;
        uint32_t p = 0, s = 0;
        if (n < a.N) {
            const int64_t b = n / a.S;
            s = a.streams[b];
            p = (a.start_dev ? (uint32_t)a.start_dev[b] : a.start) + (uint32_t)(n - b * a.S);
        }
        s_pos[tid] = p;
        s_stream[tid] = s;
    }
    __syncthreads();
    const int n = ((int)blockIdx.y * 4 + wave) * 32 + l31;     // this lane's channel
    if (n - l31 >= H) return;                                   // the whole wave, after the only barrier
    const bool n_ok = n < H;
    const float* const arow = xs + l31 * stride;
    const float* const wrow = a.W + (int64_t)(n_ok ? n : 0) * K;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int k0 = 0; k0 < K; k0 += 8) {
        const int kk = k0 + 4 * half;
        const bool ok = kk < K;
        const float4 av = *reinterpret_cast<const float4*>(arow + (ok ? kk : 0));
        const float4 wv = *reinterpret_cast<const float4*>(wrow + (ok ? kk : 0));
        acc = aura_mfma_f32_x4(ok ? av : zero, (ok && n_ok) ? wv : zero, acc);
    }
    if (!n_ok) return;
    const bool has_bias = a.b != nullptr;
    const float bias = has_bias ? a.b[n] : 0.0f;
    const float inv_T = 1.0f / (float)T;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
        const int64_t gn = row0 + row;
        if (gn >= a.N) continue;
        const float z = has_bias ? acc[r] + bias : acc[r];
        const float q = 1.0f / (1.0f + expf(-z));
        const uint32_t pos = s_pos[row], str = s_stream[row];
        float* const train = a.spikes ? a.spikes + gn * T * (int64_t)H + n : nullptr;
        int count = 0;
        for (int j = 0; 4 * j < T; ++j) {
            const Words x = bridge_philox((uint32_t)n, (uint32_t)j, pos, str, a.seed_lo, a.seed_hi);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = 4 * j + i;
                if (t < T) {
                    const float u = ((float)(x.w[i] >> 9) + 0.5f) * 1.1920928955078125e-7f;    // 2^-23: exact
                    const bool spike = u < q;                                                  // (false for a NaN q)
                    count += spike ? 1 : 0;
                    if (train) train[(int64_t)t * H] = spike ? 1.0f : 0.0f;
                }
            }
        }
        a.rate[gn * H + n] = (float)count * inv_T;
        if (a.q) a.q[gn * H + n] = q;
    }
}

inline bool misaligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) != 0; }

}  // namespace

extern "C" {

int aura_poisson_rate(const float* x, int64_t N, int64_t K, const float* W, const float* b_or_null, int64_t H, int64_t T,
                      uint64_t seed, const uint32_t* streams, int64_t rows_per_stream, int64_t start,
                      const int32_t* start_dev_or_null, float* rate, float* q_or_null, float* spikes_or_null,
                      void* stream) {
    if (N < 0 || N > AURA_BRIDGE_MAX_N) return AURA_E_INVAL;
    if (K % 4 || K < 4 || K > BR_MAX_K || H < 1 || H > AURA_BRIDGE_MAX_H || T < 1 || T > AURA_BRIDGE_MAX_T)
        return AURA_E_INVAL;
    if (rows_per_stream < 1 || N % rows_per_stream) return AURA_E_INVAL;
    if (start < 0 || start + rows_per_stream > 0x80000000LL) return AURA_E_INVAL;      // positions stay below 2^31
    if (start_dev_or_null && start != 0) return AURA_E_INVAL;
    if (!x || !W || !streams || !rate) return AURA_E_INVAL;
    if (misaligned(x, 16) || misaligned(W, 16) || misaligned(b_or_null, 4) || misaligned(streams, 4) ||
        misaligned(start_dev_or_null, 4) || misaligned(rate, 4) || misaligned(q_or_null, 4) ||
        misaligned(spikes_or_null, 4))
        return AURA_E_ALIGN;
    if (N == 0) return AURA_OK;
    BridgeArgs a;
    a.x = x; a.W = W; a.b = b_or_null; a.streams = streams; a.start_dev = start_dev_or_null;
    a.rate = rate; a.q = q_or_null; a.spikes = spikes_or_null;
    a.N = N; a.S = rows_per_stream; a.K = (int)K; a.H = (int)H; a.T = (int)T;
    a.start = (uint32_t)start; a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
    const dim3 grid((unsigned)((N + BR_ROWS - 1) / BR_ROWS), (unsigned)((H + 127) / 128));
    hipLaunchKernelGGL(poisson_rate_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return aura_check_launch();
}

}  // extern "C"
