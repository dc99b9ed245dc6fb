// aura_rowlin.hip -- a linear layer for a handful of rows (R <= 32): up to three weight matrices that share the input,
// LayerNorm in front, bias, exact GELU and a residual behind, in one launch (gfx950).
// The rule is stated once, in include/aura_hip.h ("Row linear"); the comments here are about how it is computed.
//   One wave owns CT consecutive output columns of the concatenated column range [0, N0 + N1 + N2) and all R rows of
//   them; four waves make a workgroup (sixteen from 9 rows and 2048 columns up).  A weight row is streamed once, 16
//   bytes per lane (1 KB per wave and load, contiguous), straight to registers, and serves every row: the RT x CT sums
//   live in registers.  The input rows are staged in LDS in tiles of 256 STEPS columns (a multiple of the 256 columns
//   a wave covers per load, so a lane meets its own k in ascending order across tiles; at most 64 KB).  A tile's loads
//   (the thread's share of x, its gamma and beta, the wave's weights) are issued a whole tile ahead of their use, and
//   the barriers order LDS traffic only, so they stay in flight under the previous tile's sums.  With the prologue
//   every workgroup computes the R row statistics itself (the rows are a few KB in L2) and normalises while it stages;
//   workgroup 0 also writes the normalised rows out.  A column's 64 partials meet in the xor butterfly; lane r then
//   holds row r and applies bias, GELU and residual.
// Workgroups are independent: no atomics, no flags, one pass.  RT (the power of two >= R), CT and the waves per
// workgroup are launch geometry only: an element's summation order depends on K alone.
//
// Gate epilogue (aura_row_linear_gate; the rule: "Row linear: gate epilogue").  The same kernel, instantiated a second
// time with EPI = RL_EPI_GATE: a compile-time switch, so the instantiations behind aura_row_linear are the code they
// were.  Two things differ.  The weight rows are ldw floats apart instead of K, so that the left half of a [N][2K]
// parameter is streamed in place (a row's 16-byte units stay aligned: ldw % 4 == 0).  And lane r, which holds row r's
// sum after the butterfly, loads its u, c and res element and finishes y = res + sigmoid(t + u) c: three more loads
// and one expf per output element, behind the same dot product, in the same launch.
//
// GIF epilogue (aura_row_linear_gif; the rule: "Row linear: GIF epilogue").  EPI = RL_EPI_GIF_TI / RL_EPI_GIF_TM: the
// current t = dot + b feeds the GIF step of aura_neuron.hip (the one GifModel of aura_gif_model.inl, so the bits are
// aura_gif_run's) without a round trip through memory.  Time-invariant: lane r, which holds row r's current, runs its T
// steps from fresh state and writes T spikes.  Time-major: the rows tok T .. tok T + T - 1 are a token's T steps; every
// lane of the token reads them in order with __shfl (all 64 lanes take part: the branch around the loop is
// wave-uniform) and runs the same T steps, the token's first lane divides the spike sum by T and, with the mix,
// finishes res + ((1 - g) m + g mean), g = sigmoid(*gate) read from device memory.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/aura_hip.h"
#include "aura_common.inl"

namespace {

#include "aura_gif_model.inl"

// Waves per workgroup.  Every workgroup stages all R rows, so its cost in L2 reads is R K per workgroup: at 16 and 32
// rows sixteen waves share a tile where there are columns enough for it (a quarter of the L2 reads per output column
// and of the staging registers per lane); with few columns four waves keep more CUs at work.
constexpr int RL_WAVES = 4;
constexpr int RL_WAVES_WIDE = 16;
constexpr int RL_MAX_ROWS = AURA_ROW_LINEAR_MAX_ROWS;
constexpr int RL_MAX_K = AURA_ROW_LINEAR_MAX_K;
constexpr int RL_MAX_NORM_K = 2048;
constexpr int RL_NORM_UNITS = RL_MAX_NORM_K / 256;      // float4 units of a row per lane in the prologue, at most

typedef float rl_v4 __attribute__((ext_vector_type(4)));

struct RowLinArgs {
    const float* x;                     // [R][K]
    const float* W[3];                  // [N_j][K]
    const float* b[3];                  // [N_j] or NULL
    float* y[3];                        // [R][N_j]
    const float* gamma;                 // [K] or NULL (no prologue)
    const float* beta;                  // [K]
    const float* res;                   // [R][N_0] or NULL
    float* xh;                          // [R][K] or NULL
    int N[3];
    int Nt;                             // N_0 + N_1 + N_2
    int R, K;
    int gelu, nontemporal;
    float eps;
    // the gate epilogue's (EPI == RL_EPI_GATE; unused otherwise)
    const float* gate_u;                // [R][N_0]
    const float* gate_c;                // [R][N_0]
    int64_t ldw;                        // floats between the rows of W_0, >= K
    // the GIF epilogues' (EPI == RL_EPI_GIF_TI / RL_EPI_GIF_TM; unused otherwise)
    float gif_decay, gif_L, gif_alpha, gif_thr;
    int gif_T;
    const float* mix_m;                 // [R / T][N_0] or NULL (no mix: the mean is written); with it res is [R / T][N_0]
    const float* mix_gate;              // one float
};

constexpr int RL_EPI_PLAIN = 0;         // bias, GELU, residual
constexpr int RL_EPI_GATE = 1;          // bias, then res + sigmoid(t + u) c
constexpr int RL_EPI_GIF_TI = 2;        // bias, then T GIF steps on the row's own current: spikes [R][T][N]
constexpr int RL_EPI_GIF_TM = 3;        // bias, then a token's T rows through the GIF: the T-mean [R / T][N], or the mix

__device__ __forceinline__ float rl_wave_sum(float s) {
    s = s + __shfl_xor(s, 32);
    s = s + __shfl_xor(s, 16);
    s = s + __shfl_xor(s, 8);
    s = s + __shfl_xor(s, 4);
    s = s + __shfl_xor(s, 2);
    s = s + __shfl_xor(s, 1);
    return s;
}

__device__ __forceinline__ float rl_gelu(float t) {
    return (0.5f * t) * (1.0f + erff(t * 0.70710678118654752440f));
}

// (mean, rstd) of the rows wave, wave + WV, ..: the wave takes its rows together, so that their loads and their
// butterflies overlap instead of queueing behind one another (a row after a row would cost R / 4 memory latencies).
// Every lane takes part and gets the same bits.  A lane past the row's end, and a row past R, load a clamped address;
// the lane contributes zeros (s + 0 == s) and the row is not kept: no load sits behind a branch.  The second pass reads
// the row again (from L2) instead of holding it in registers.
template <int RW, int WV>
__device__ __forceinline__ void rl_row_stats(const RowLinArgs& a, int wave, int lane, float2* stats) {
    const float4* const x4 = reinterpret_cast<const float4*>(a.x);
    const int U = a.K / 4;
    const float4* row[RW];
#pragma unroll
    for (int m = 0; m < RW; ++m) {
        const int r = wave + WV * m;
        row[m] = x4 + (int64_t)(r < a.R ? r : a.R - 1) * U;
    }
    float s[RW], mu[RW], q[RW];
#pragma unroll
    for (int m = 0; m < RW; ++m) s[m] = q[m] = 0.0f;
#pragma unroll 2
    for (int i = 0; i < RL_NORM_UNITS; ++i) {
        if (64 * i >= U) break;                                         // wave-uniform
        const int u = lane + 64 * i;
        const bool live = u < U;
#pragma unroll
        for (int m = 0; m < RW; ++m) {
            const float4 v = row[m][live ? u : U - 1];
            s[m] = s[m] + (live ? v.x : 0.0f);
            s[m] = s[m] + (live ? v.y : 0.0f);
            s[m] = s[m] + (live ? v.z : 0.0f);
            s[m] = s[m] + (live ? v.w : 0.0f);
        }
    }
#pragma unroll
    for (int m = 0; m < RW; ++m) mu[m] = rl_wave_sum(s[m]) / (float)a.K;
#pragma unroll 2
    for (int i = 0; i < RL_NORM_UNITS; ++i) {
        if (64 * i >= U) break;
        const int u = lane + 64 * i;
        const bool live = u < U;
#pragma unroll
        for (int m = 0; m < RW; ++m) {
            const float4 v = row[m][live ? u : U - 1];
            const float dx = live ? v.x - mu[m] : 0.0f, dy = live ? v.y - mu[m] : 0.0f;
            const float dz = live ? v.z - mu[m] : 0.0f, dw = live ? v.w - mu[m] : 0.0f;
            q[m] = q[m] + dx * dx;
            q[m] = q[m] + dy * dy;
            q[m] = q[m] + dz * dz;
            q[m] = q[m] + dw * dw;
        }
    }
#pragma unroll
    for (int m = 0; m < RW; ++m) {
        const float var = rl_wave_sum(q[m]) / (float)a.K;
        const int r = wave + WV * m;
        if (lane == 0 && r < a.R) stats[r] = make_float2(mu[m], 1.0f / sqrtf(var + a.eps));
    }
}

// A barrier that orders the workgroup's LDS traffic only: global loads issued before it stay in flight across it
// (__syncthreads() would wait for them, and the next tile's prefetch would be waited for at once).
__device__ __forceinline__ void rl_lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

template <int RT, int WAVES>
struct RowLinTile {
    static constexpr int STEPS = 64 / RT < 4 ? 64 / RT : 4;             // weight loads per lane, column and tile
    static constexpr int KC4 = 64 * STEPS;                              // float4 units of a row per tile
    static constexpr int WV = WAVES;                                    // waves per workgroup
    static constexpr int NX = RT * KC4 / (64 * WV);                     // float4 units a thread stages per tile
    static constexpr int ROW_STEP = 64 * WV / KC4;                      // rows between a thread's units
    static constexpr int LDS_BYTES = RT * KC4 * 16 + RT * 8;            // the tile (at most 64 KB) and the row statistics
};

// one tile's loads, issued a whole tile ahead of their use: the thread's share of the x tile (with the prologue also
// its gamma and beta unit: a thread stages one column unit of several rows) and the wave's weights
template <int RT, int CT, int WAVES>
struct RowLinRegs {
    typedef RowLinTile<RT, WAVES> T;
    float4 x[T::NX], gm, bt;
    rl_v4 w[T::STEPS][CT];

    // Every load takes a clamped address, and what it returns is looked at only where it is used, a tile later (the
    // staging and the sums decide there whether the unit counts): no load sits behind a per-lane branch and nothing
    // waits for one here, so a tile's loads are in flight together under the previous tile's sums.
    __device__ __forceinline__ void load(const RowLinArgs& a, const rl_v4* const (&wrow)[CT], int u0, int lane) {
        const int U = a.K / 4;
        const int u = u0 + threadIdx.x % T::KC4, r0 = threadIdx.x / T::KC4;
        const int uc = u < U ? u : U - 1;
        const float4* const x4 = reinterpret_cast<const float4*>(a.x);
        if (a.gamma) {
            gm = reinterpret_cast<const float4*>(a.gamma)[uc];
            bt = reinterpret_cast<const float4*>(a.beta)[uc];
        }
#pragma unroll
        for (int m = 0; m < T::NX; ++m) {
            const int r = r0 + m * T::ROW_STEP;
            x[m] = x4[(int64_t)(r < a.R ? r : a.R - 1) * U + uc];
        }
#pragma unroll
        for (int s = 0; s < T::STEPS; ++s) {
            if (u0 + 64 * s < U) {                                      // wave-uniform
                const int uw = u0 + 64 * s + lane;
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    const rl_v4* const p = wrow[c] + (uw < U ? uw : U - 1);
                    w[s][c] = a.nontemporal ? __builtin_nontemporal_load(p) : *p;
                }
            }
        }
    }
};

template <int RT, int CT, int WAVES, int EPI = RL_EPI_PLAIN>
__global__ __launch_bounds__(64 * WAVES) void row_linear_kernel(const RowLinArgs a) {
    typedef RowLinTile<RT, WAVES> T;
    constexpr int STEPS = T::STEPS, KC4 = T::KC4, WV = T::WV;
    extern __shared__ float4 rl_lds[];
    float4* const tile = rl_lds;                                        // [RT][KC4]
    float2* const stats = reinterpret_cast<float2*>(rl_lds + RT * KC4); // [RT]: mean, rstd
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int U = a.K / 4;

    // this wave's columns; a column past the end repeats the last one and is not stored
    const int64_t g0 = ((int64_t)blockIdx.x * WV + wave) * CT;
    const rl_v4* wrow[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        int64_t g = g0 + c < a.Nt ? g0 + c : a.Nt - 1;
        int j = 0;
        if (g >= a.N[0]) { g -= a.N[0]; j = 1; }
        if (j == 1 && g >= a.N[1]) { g -= a.N[1]; j = 2; }
        wrow[c] = reinterpret_cast<const rl_v4*>(a.W[j] + g * (EPI == RL_EPI_GATE ? a.ldw : (int64_t)a.K));
    }

    RowLinRegs<RT, CT, WAVES> cur, nxt;
    cur.load(a, wrow, 0, lane);                                         // in flight under the row statistics

    if (a.gamma) {
        rl_row_stats<(RT + WV - 1) / WV, WV>(a, wave, lane, stats);
        rl_lds_barrier();
    }

    float acc[RT][CT];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[r][c] = 0.0f;

    float4* const xh4 = (a.xh && blockIdx.x == 0) ? reinterpret_cast<float4*>(a.xh) : nullptr;
    const int su = threadIdx.x % KC4, sr0 = threadIdx.x / KC4;          // the unit and first row this thread stages

    for (int u0 = 0; u0 < U; u0 += KC4) {
        if (u0 > 0) rl_lds_barrier();                                   // the previous tile has been read
#pragma unroll
        for (int m = 0; m < T::NX; ++m) {
            const int r = sr0 + m * T::ROW_STEP;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);              // rows past R and units past K are staged as zeros
            if (r < a.R && u0 + su < U) {
                v = cur.x[m];
                if (a.gamma) {
                    const float2 st = stats[r];
                    v.x = ((v.x - st.x) * st.y) * cur.gm.x + cur.bt.x;
                    v.y = ((v.y - st.x) * st.y) * cur.gm.y + cur.bt.y;
                    v.z = ((v.z - st.x) * st.y) * cur.gm.z + cur.bt.z;
                    v.w = ((v.w - st.x) * st.y) * cur.gm.w + cur.bt.w;
                    if (xh4) xh4[(int64_t)r * U + u0 + su] = v;
                }
            }
            tile[r * KC4 + su] = v;
        }
        if (u0 + KC4 < U) nxt.load(a, wrow, u0 + KC4, lane);            // the next tile's loads run under this tile's sums
        rl_lds_barrier();
#pragma unroll
        for (int s = 0; s < STEPS; ++s) {
            if (u0 + 64 * s < U) {                                      // wave-uniform
                // a lane past K holds a clamped weight: zero it; its x is staged as zero too, and fmaf(0, 0, t) == t
                const bool live = u0 + 64 * s + lane < U;
                rl_v4 w[CT];
#pragma unroll
                for (int c = 0; c < CT; ++c) w[c] = live ? cur.w[s][c] : (rl_v4)(0.0f);
#pragma unroll
                for (int r = 0; r < RT; ++r) {
                    const float4 xv = tile[r * KC4 + 64 * s + lane];
#pragma unroll
                    for (int c = 0; c < CT; ++c) {
                        float t = acc[r][c];
                        t = fmaf(xv.x, w[c].x, t);
                        t = fmaf(xv.y, w[c].y, t);
                        t = fmaf(xv.z, w[c].z, t);
                        t = fmaf(xv.w, w[c].w, t);
                        acc[r][c] = t;
                    }
                }
            }
        }
        cur = nxt;
    }

    // the butterfly leaves every sum in every lane; lane r keeps row r and finishes it
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        float mine = 0.0f;
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const float v = rl_wave_sum(acc[r][c]);
            if (lane == r) mine = v;
        }
        int64_t g = g0 + c;
        if constexpr (EPI == RL_EPI_GIF_TI || EPI == RL_EPI_GIF_TM) {
            if (g < a.Nt) {                                             // wave-uniform: every lane reaches the shuffles
                float t = mine;
                if (a.b[0]) t = t + a.b[0][g];
                const GifModel<false> gif{a.gif_decay, a.gif_L, a.gif_alpha, a.gif_thr};
                GifModel<false>::Lane st;
                st.s0 = 0.0f;
                st.s1 = a.gif_thr;
                const int nt = a.gif_T;                                 // the neuron loop's steps
                if constexpr (EPI == RL_EPI_GIF_TI) {
                    if (lane < a.R) {
                        float* const o = a.y[0] + (int64_t)lane * nt * a.N[0] + g;
                        for (int tt = 0; tt < nt; ++tt) o[(int64_t)tt * a.N[0]] = gif.step(st, t);
                    }
                } else {
                    const int first = lane - lane % nt;                 // the token's first row
                    float acc = 0.0f;
                    for (int tt = 0; tt < nt; ++tt) {
                        const int src = first + tt;
                        acc += gif.step(st, __shfl(t, src < 64 ? src : 63));
                    }
                    if (lane < a.R && lane == first) {
                        float y = acc / (float)nt;
                        const int64_t o = (int64_t)(lane / nt) * a.N[0] + g;
                        if (a.mix_m) {
                            const float gt = 1.0f / (1.0f + expf(-a.mix_gate[0]));
                            const float left = (1.0f - gt) * a.mix_m[o];
                            const float right = gt * y;
                            y = a.res[o] + (left + right);
                        }
                        a.y[0][o] = y;
                    }
                }
            }
            continue;
        }
        if (g < a.Nt && lane < a.R) {
            int j = 0;
            if (g >= a.N[0]) { g -= a.N[0]; j = 1; }
            if (j == 1 && g >= a.N[1]) { g -= a.N[1]; j = 2; }
            float t = mine;
            if (a.b[j]) t = t + a.b[j][g];
            const int64_t o = (int64_t)lane * a.N[j] + g;
            if constexpr (EPI == RL_EPI_GATE) {
                const float act = t + a.gate_u[o];
                const float s = 1.0f / (1.0f + expf(-act));
                t = a.res[o] + s * a.gate_c[o];
            } else {
                if (a.gelu) t = rl_gelu(t);
                if (a.res) t = t + a.res[o];
            }
            a.y[j][o] = t;
        }
    }
}

inline void rl_no_gif(RowLinArgs& a) {
    a.gif_decay = a.gif_L = a.gif_alpha = a.gif_thr = 0.0f;
    a.gif_T = 0;
    a.mix_m = a.mix_gate = nullptr;
}

inline bool misaligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) != 0; }

template <int RT, int CT, int WV, int EPI>
int rl_launch_geometry(const RowLinArgs& a, hipStream_t s) {
    constexpr int lds = RowLinTile<RT, WV>::LDS_BYTES;
    if (lds > 48 * 1024) {                                              // above the default dynamic limit
        const int rc = aura_ensure_lds_attr(reinterpret_cast<const void*>(&row_linear_kernel<RT, CT, WV, EPI>), lds);
        if (rc != AURA_OK) return rc;
    }
    const int64_t waves = ((int64_t)a.Nt + CT - 1) / CT;
    const dim3 grid((unsigned)((waves + WV - 1) / WV)), block(64 * WV);
    hipLaunchKernelGGL((row_linear_kernel<RT, CT, WV, EPI>), grid, block, lds, s, a);
    return AURA_OK;
}

// The launch geometry: a choice of speed only, an element's summation order does not depend on it.
template <int RT, int EPI = RL_EPI_PLAIN>
int rl_launch(const RowLinArgs& a, hipStream_t s) {
    if (RT >= 16) {
        if (a.Nt >= 2048) return rl_launch_geometry<RT, 1, RT >= 16 ? RL_WAVES_WIDE : RL_WAVES, EPI>(a, s);
        return rl_launch_geometry<RT, 1, RL_WAVES, EPI>(a, s);
    }
    // more columns per wave only where enough waves remain to fill the device, and only while the RT x CT sums and
    // the two tiles of loads in flight leave registers for two workgroups a CU
    if (a.Nt >= 8192 && RT <= 4) return rl_launch_geometry<RT, RT <= 4 ? 4 : 1, RL_WAVES, EPI>(a, s);
    if (a.Nt >= 2048 && RT <= 8) return rl_launch_geometry<RT, RT <= 8 ? 2 : 1, RL_WAVES, EPI>(a, s);
    return rl_launch_geometry<RT, 1, RL_WAVES, EPI>(a, s);
}

template <int EPI>
int rl_launch_rows(const RowLinArgs& a, hipStream_t s) {
    if (a.R <= 1) return rl_launch<1, EPI>(a, s);
    if (a.R <= 2) return rl_launch<2, EPI>(a, s);
    if (a.R <= 4) return rl_launch<4, EPI>(a, s);
    if (a.R <= 8) return rl_launch<8, EPI>(a, s);
    if (a.R <= 16) return rl_launch<16, EPI>(a, s);
    return rl_launch<32, EPI>(a, s);
}

}  // namespace

extern "C" {

int aura_row_linear(const float* x, int64_t R, int64_t K, const float* W0, const float* b0_or_null, float* y0,
                    int64_t N0, const float* W1_or_null, const float* b1_or_null, float* y1_or_null, int64_t N1,
                    const float* W2_or_null, const float* b2_or_null, float* y2_or_null, int64_t N2,
                    const float* gamma_or_null, const float* beta_or_null, float eps, float* xh_or_null, int gelu,
                    const float* res_or_null, int nontemporal, void* stream) {
    if (R < 1 || R > RL_MAX_ROWS || K < 4 || K > RL_MAX_K || K % 4 != 0) return AURA_E_INVAL;
    if (!x || !W0 || !y0 || N0 < 1) return AURA_E_INVAL;
    if (!W1_or_null && (W2_or_null || b1_or_null || y1_or_null || N1 != 0)) return AURA_E_INVAL;
    if (!W2_or_null && (b2_or_null || y2_or_null || N2 != 0)) return AURA_E_INVAL;
    if (W1_or_null && (!y1_or_null || N1 < 1)) return AURA_E_INVAL;
    if (W2_or_null && (!y2_or_null || N2 < 1)) return AURA_E_INVAL;
    if (N0 > 0x7fffffff || N1 > 0x7fffffff || N2 > 0x7fffffff || N0 + N1 + N2 > 0x7fffffff) return AURA_E_INVAL;
    if ((gamma_or_null == nullptr) != (beta_or_null == nullptr)) return AURA_E_INVAL;
    if (gamma_or_null && (K > RL_MAX_NORM_K || !(eps >= 0.0f))) return AURA_E_INVAL;
    if (xh_or_null && !gamma_or_null) return AURA_E_INVAL;
    if (res_or_null && W1_or_null) return AURA_E_INVAL;
    if (misaligned(x, 16) || misaligned(W0, 16) || misaligned(W1_or_null, 16) || misaligned(W2_or_null, 16) ||
        misaligned(gamma_or_null, 16) || misaligned(beta_or_null, 16) || misaligned(xh_or_null, 16) ||
        misaligned(b0_or_null, 4) || misaligned(b1_or_null, 4) || misaligned(b2_or_null, 4) || misaligned(y0, 4) ||
        misaligned(y1_or_null, 4) || misaligned(y2_or_null, 4) || misaligned(res_or_null, 4))
        return AURA_E_ALIGN;
    RowLinArgs a;
    a.x = x;
    a.W[0] = W0; a.W[1] = W1_or_null; a.W[2] = W2_or_null;
    a.b[0] = b0_or_null; a.b[1] = b1_or_null; a.b[2] = b2_or_null;
    a.y[0] = y0; a.y[1] = y1_or_null; a.y[2] = y2_or_null;
    a.N[0] = (int)N0; a.N[1] = (int)N1; a.N[2] = (int)N2;
    a.Nt = (int)(N0 + N1 + N2);
    a.gamma = gamma_or_null; a.beta = beta_or_null; a.res = res_or_null; a.xh = xh_or_null;
    a.R = (int)R; a.K = (int)K;
    a.gelu = gelu != 0; a.nontemporal = nontemporal != 0;
    a.eps = eps;
    a.gate_u = a.gate_c = nullptr;
    a.ldw = K;
    rl_no_gif(a);
    const int rc = rl_launch_rows<RL_EPI_PLAIN>(a, static_cast<hipStream_t>(stream));
    if (rc != AURA_OK) return rc;
    return aura_check_launch();
}

int aura_row_linear_gate(const float* x, int64_t R, int64_t K, const float* W, int64_t ldw, const float* b_or_null,
                         const float* u, const float* c, const float* res, float* y, int64_t N, int nontemporal,
                         void* stream) {
    if (R < 1 || R > RL_MAX_ROWS || K < 4 || K > RL_MAX_K || K % 4 != 0) return AURA_E_INVAL;
    if (!x || !W || !u || !c || !res || !y || N < 1 || N > 0x7fffffff) return AURA_E_INVAL;
    if (ldw < K || ldw % 4 != 0) return AURA_E_INVAL;
    if (misaligned(x, 16) || misaligned(W, 16) || misaligned(b_or_null, 4) || misaligned(u, 4) || misaligned(c, 4) ||
        misaligned(res, 4) || misaligned(y, 4))
        return AURA_E_ALIGN;
    RowLinArgs a;
    a.x = x;
    a.W[0] = W; a.W[1] = nullptr; a.W[2] = nullptr;
    a.b[0] = b_or_null; a.b[1] = nullptr; a.b[2] = nullptr;
    a.y[0] = y; a.y[1] = nullptr; a.y[2] = nullptr;
    a.N[0] = (int)N; a.N[1] = 0; a.N[2] = 0;
    a.Nt = (int)N;
    a.gamma = nullptr; a.beta = nullptr; a.res = res; a.xh = nullptr;
    a.R = (int)R; a.K = (int)K;
    a.gelu = 0; a.nontemporal = nontemporal != 0;
    a.eps = 0.0f;
    a.gate_u = u; a.gate_c = c;
    a.ldw = ldw;
    rl_no_gif(a);
    const int rc = rl_launch_rows<RL_EPI_GATE>(a, static_cast<hipStream_t>(stream));
    if (rc != AURA_OK) return rc;
    return aura_check_launch();
}

int aura_row_linear_gif(const float* x, int64_t R, int64_t K, const float* W, const float* b_or_null, float* out,
                        int64_t N, int64_t T, float decay, int L, float alpha, float threshold, int time_major,
                        const float* res_or_null, const float* m_or_null, const float* gate_or_null, int nontemporal,
                        void* stream) {
    if (R < 1 || R > RL_MAX_ROWS || K < 4 || K > RL_MAX_K || K % 4 != 0) return AURA_E_INVAL;
    if (!x || !W || !out || N < 1 || N > 0x7fffffff) return AURA_E_INVAL;
    if (T < 1 || T > RL_MAX_ROWS || L < 1) return AURA_E_INVAL;
    if (time_major && R % T != 0) return AURA_E_INVAL;
    const int mixed = (res_or_null != nullptr) + (m_or_null != nullptr) + (gate_or_null != nullptr);
    if (mixed != 0 && (mixed != 3 || !time_major)) return AURA_E_INVAL;
    if (misaligned(x, 16) || misaligned(W, 16) || misaligned(b_or_null, 4) || misaligned(out, 4) ||
        misaligned(res_or_null, 4) || misaligned(m_or_null, 4) || misaligned(gate_or_null, 4))
        return AURA_E_ALIGN;
    RowLinArgs a;
    a.x = x;
    a.W[0] = W; a.W[1] = nullptr; a.W[2] = nullptr;
    a.b[0] = b_or_null; a.b[1] = nullptr; a.b[2] = nullptr;
    a.y[0] = out; a.y[1] = nullptr; a.y[2] = nullptr;
    a.N[0] = (int)N; a.N[1] = 0; a.N[2] = 0;
    a.Nt = (int)N;
    a.gamma = nullptr; a.beta = nullptr; a.res = res_or_null; a.xh = nullptr;
    a.R = (int)R; a.K = (int)K;
    a.gelu = 0; a.nontemporal = nontemporal != 0;
    a.eps = 0.0f;
    a.gate_u = a.gate_c = nullptr;
    a.ldw = K;
    a.gif_decay = decay; a.gif_L = (float)L; a.gif_alpha = alpha; a.gif_thr = threshold;
    a.gif_T = (int)T;
    a.mix_m = m_or_null; a.mix_gate = gate_or_null;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = time_major ? rl_launch_rows<RL_EPI_GIF_TM>(a, s) : rl_launch_rows<RL_EPI_GIF_TI>(a, s);
    if (rc != AURA_OK) return rc;
    return aura_check_launch();
}

}  // extern "C"
