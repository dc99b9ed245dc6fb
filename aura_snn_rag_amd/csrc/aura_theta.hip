// aura_theta.hip -- theta-gamma positions: the phase-code table, and residual add + LayerNorm over it in one launch; the
// backward in a main and a finish launch (gfx950).
// The rule is stated once, in include/aura_hip.h ("Theta-gamma"); the comments here are about how it is computed.
//   table      one thread per (row, column): the only place a sine or cosine is evaluated, R * D times per call (R = S
//              when the batch shares its positions), never per token.  sinf / cosf are the accurate device functions
//              with the full range reduction; the file is built with -ffp-contract=off like every other.
//   rows       forward and backward: one wave owns a token, a workgroup is four waves.  The row sits in registers as NU
//              units per lane (unit u = 64 j + lane; a unit is a float4 when D % 4 == 0, else a float), so a lane's
//              elements ascend in d and the two row sums are: the lane's own elements in that order, then the xor
//              butterfly 32, 16, 8, 4, 2, 1.  An element beyond D holds 0 and adds 0.
//   forward    reads the token's x row and its table row, writes y, mean and rstd; h = x + pe lives in registers only.
//   backward   a wave walks a contiguous run of tokens in ascending order and carries five column partials per element
//              (g_w, g_b, g_theta, g_gamma, g_amp); the four waves of a workgroup are added in wave order through one
//              LDS image (wave 0 stores, waves 1 .. 3 add in turn), the last wave writes row g of partials [G][5][D].
//              G = theta_groups(N) depends on N alone.
//   finish     a thread per (eighth of G, column) adds its partials in ascending g; the eight segments in order.
// No atomics anywhere; nothing depends on the grid or on the device.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/aura_hip.h"
#include "aura_common.inl"

namespace {

constexpr int THETA_WAVES = 4;          // tokens per workgroup (forward); waves whose partials a workgroup adds
constexpr int THETA_MAX_D = 2048;
constexpr int THETA_STATS = 5;          // g_w, g_b, g_theta, g_gamma, g_amp
constexpr int THETA_FINISH_COLS = 32;
constexpr int THETA_FINISH_SEGS = 8;
constexpr float THETA_TWO_PI = 6.28318530717958647692f;

struct ThetaTableArgs {
    const float* pos;                   // [R] or NULL: float(start + r)
    const float* th;                    // [D]
    const float* ga;                    // [D]
    const float* amp;                   // [D]
    float* pe;                          // [R][D] or NULL
    float* d_th;                        // [R][D] or NULL (the three together)
    float* d_ga;
    float* d_amp;
    int64_t start, R;
    int D;
    float denom, ratio;
};

struct ThetaNormArgs {
    const float* x;                     // [N][D]
    const float* table;                 // [R][D]
    const float* w;                     // [D]
    const float* b;                     // [D]
    float* y;                           // [N][D]
    float* mean;                        // [N]
    float* rstd;                        // [N]
    int64_t N, S;
    int D, per_token;                   // per_token: table row n, else n % S
    float eps;
};

struct ThetaBwdArgs {
    const float* g_y;                   // [N][D]
    const float* x;                     // [N][D]
    const float* table;                 // [R][D]
    const float* d_th;                  // [R][D] or NULL (the three together)
    const float* d_ga;
    const float* d_amp;
    const float* mean;                  // [N]
    const float* rstd;                  // [N]
    const float* w;                     // [D]
    float* g_x;                         // [N][D]
    float* partials;                    // [G][5][D] or NULL: no column sums wanted
    int64_t N, S, chunk;                // chunk: tokens per wave
    int D, per_token;
};

// how many workgroups share the tokens of the backward: a function of N alone
inline int64_t theta_groups(int64_t N) {
    const int64_t g = (N + 15) / 16;
    return g < 1 ? 1 : (g > 1024 ? 1024 : g);
}

__global__ __launch_bounds__(256) void theta_gamma_table_kernel(const ThetaTableArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.R * a.D) return;
    const int64_t r = i / a.D;
    const int d = (int)(i - r * a.D);
    const float p = a.pos ? a.pos[r] : (float)(a.start + r);
    const float phi = (p / a.denom) * THETA_TWO_PI;
    const float ta = phi + a.th[d];
    const float tg = phi * a.ratio + a.ga[d];
    const float sa = sinf(ta), ca = cosf(ta), sg = sinf(tg);
    const float A = (ca + 1.0f) * 0.5f;
    const float q = sa + 0.5f * (A * sg);
    const float amp = a.amp[d];
    if (a.pe) a.pe[i] = q * amp;
    if (a.d_th) {
        const float cg = cosf(tg);
        a.d_th[i] = amp * (ca - (0.25f * sa) * sg);
        a.d_ga[i] = amp * ((0.5f * A) * cg);
        a.d_amp[i] = q;
    }
}

// A row [D] in registers: unit j of a lane is unit 64 j + lane of the row, a float4 (VEC) or a float.
template <int NU, bool VEC> struct ThetaRow {
    static constexpr int W = VEC ? 4 : 1;
    static constexpr int E = NU * W;    // elements per lane
    static __device__ __forceinline__ void load(const float* row, int D, int lane, float (&v)[E]) {
        const int U = VEC ? D / 4 : D;
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            const int u = j * 64 + lane;
            if constexpr (VEC) {
                float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (u < U) t = reinterpret_cast<const float4*>(row)[u];
                v[4 * j] = t.x; v[4 * j + 1] = t.y; v[4 * j + 2] = t.z; v[4 * j + 3] = t.w;
            } else {
                v[j] = u < U ? row[u] : 0.0f;
            }
        }
    }
    static __device__ __forceinline__ void store(float* row, int D, int lane, const float (&v)[E]) {
        const int U = VEC ? D / 4 : D;
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            const int u = j * 64 + lane;
            if (u < U) {
                if constexpr (VEC)
                    reinterpret_cast<float4*>(row)[u] = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
                else
                    row[u] = v[j];
            }
        }
    }
    // is element e of this lane inside the row?
    static __device__ __forceinline__ bool live(int e, int D, int lane) {
        return ((e / W) * 64 + lane) * W + (e % W) < D;
    }
};

__device__ __forceinline__ float theta_wave_sum(float s) {
    s = s + __shfl_xor(s, 32);
    s = s + __shfl_xor(s, 16);
    s = s + __shfl_xor(s, 8);
    s = s + __shfl_xor(s, 4);
    s = s + __shfl_xor(s, 2);
    s = s + __shfl_xor(s, 1);
    return s;
}

template <int NU, bool VEC>
__global__ __launch_bounds__(64 * THETA_WAVES) void theta_gamma_norm_kernel(const ThetaNormArgs a) {
    typedef ThetaRow<NU, VEC> Row;
    constexpr int E = Row::E;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n = (int64_t)blockIdx.x * THETA_WAVES + wave;
    if (n >= a.N) return;
    const int D = a.D;
    const int64_t trow = a.per_token ? n : n % a.S;
    float h[E], t[E];
    Row::load(a.x + n * D, D, lane, h);
    Row::load(a.table + trow * D, D, lane, t);
    float s = 0.0f;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        h[e] = h[e] + t[e];
        s = s + h[e];
    }
    const float mu = theta_wave_sum(s) / (float)D;
    float q = 0.0f;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        h[e] = h[e] - mu;
        q = q + (Row::live(e, D, lane) ? h[e] * h[e] : 0.0f);
    }
    const float var = theta_wave_sum(q) / (float)D;
    const float rstd = 1.0f / sqrtf(var + a.eps);
    Row::load(a.w, D, lane, t);
#pragma unroll
    for (int e = 0; e < E; ++e) h[e] = (h[e] * rstd) * t[e];
    Row::load(a.b, D, lane, t);
#pragma unroll
    for (int e = 0; e < E; ++e) h[e] = h[e] + t[e];
    Row::store(a.y + n * D, D, lane, h);
    if (lane == 0) {
        a.mean[n] = mu;
        a.rstd[n] = rstd;
    }
}

template <int NU, bool VEC, bool DERIV>
__global__ __launch_bounds__(64 * THETA_WAVES) void theta_gamma_norm_backward_kernel(const ThetaBwdArgs a) {
    typedef ThetaRow<NU, VEC> Row;
    constexpr int E = Row::E;
    constexpr int NS = DERIV ? THETA_STATS : 2;
    __shared__ float s_part[NS][E * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int D = a.D;
    const int64_t t0 = ((int64_t)blockIdx.x * THETA_WAVES + wave) * a.chunk;
    const int64_t t1 = t0 + a.chunk < a.N ? t0 + a.chunk : a.N;
    const bool sums = a.partials != nullptr;                            // uniform over the grid

    float acc[NS][E];
#pragma unroll
    for (int k = 0; k < NS; ++k)
#pragma unroll
        for (int e = 0; e < E; ++e) acc[k][e] = 0.0f;

    for (int64_t n = t0; n < t1; ++n) {
        const int64_t trow = a.per_token ? n : n % a.S;
        const float mu = a.mean[n], rstd = a.rstd[n];
        float nn[E], g[E], t[E];
        Row::load(a.x + n * D, D, lane, nn);
        Row::load(a.table + trow * D, D, lane, t);
        Row::load(a.g_y + n * D, D, lane, g);
#pragma unroll
        for (int e = 0; e < E; ++e) nn[e] = ((nn[e] + t[e]) - mu) * rstd;     // h, then n, as the forward rounded them
        if (sums) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                acc[0][e] = acc[0][e] + g[e] * nn[e];
                acc[1][e] = acc[1][e] + g[e];
            }
        }
        Row::load(a.w, D, lane, t);
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            g[e] = t[e] * g[e];                                              // wg; 0 beyond the row
            s1 = s1 + g[e];
            s2 = s2 + (Row::live(e, D, lane) ? g[e] * nn[e] : 0.0f);
        }
        const float c1 = theta_wave_sum(s1) / (float)D;
        const float c2 = theta_wave_sum(s2) / (float)D;
#pragma unroll
        for (int e = 0; e < E; ++e) g[e] = rstd * ((g[e] - c1) - nn[e] * c2);   // g_h = g_x
        Row::store(a.g_x + n * D, D, lane, g);
        if constexpr (DERIV) {
            if (sums) {
                Row::load(a.d_th + trow * D, D, lane, t);
#pragma unroll
                for (int e = 0; e < E; ++e) acc[2][e] = acc[2][e] + g[e] * t[e];
                Row::load(a.d_ga + trow * D, D, lane, t);
#pragma unroll
                for (int e = 0; e < E; ++e) acc[3][e] = acc[3][e] + g[e] * t[e];
                Row::load(a.d_amp + trow * D, D, lane, t);
#pragma unroll
                for (int e = 0; e < E; ++e) acc[4][e] = acc[4][e] + g[e] * t[e];
            }
        }
    }
    if (!sums) return;                                                   // every wave alike: no barrier is skipped

    // the workgroup's partials: ((wave 0 + wave 1) + wave 2) + wave 3
    for (int turn = 0; turn < THETA_WAVES; ++turn) {
        if (wave == turn) {
#pragma unroll
            for (int k = 0; k < NS; ++k)
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    if (turn > 0) acc[k][e] = s_part[k][e * 64 + lane] + acc[k][e];
                    if (turn < THETA_WAVES - 1) s_part[k][e * 64 + lane] = acc[k][e];
                }
        }
        if (turn < THETA_WAVES - 1) __syncthreads();
    }
    if (wave == THETA_WAVES - 1) {
        float* const out = a.partials + (int64_t)blockIdx.x * THETA_STATS * D;
#pragma unroll
        for (int k = 0; k < NS; ++k) Row::store(out + (int64_t)k * D, D, lane, acc[k]);
    }
}

// grads[c] = sum over g of partials[g][c], c < C = ns * D (the first ns of the five rows of a group)
__global__ __launch_bounds__(THETA_FINISH_COLS * THETA_FINISH_SEGS) void theta_gamma_finish_kernel(
    const float* partials, float* grads, int64_t G, int C, int D) {
    __shared__ float s_seg[THETA_FINISH_SEGS][THETA_FINISH_COLS];
    const int col = threadIdx.x & (THETA_FINISH_COLS - 1), seg = threadIdx.x / THETA_FINISH_COLS;
    const int c = blockIdx.x * THETA_FINISH_COLS + col;
    const int64_t per = (G + THETA_FINISH_SEGS - 1) / THETA_FINISH_SEGS;
    const int64_t g0 = seg * per, g1 = g0 + per < G ? g0 + per : G;
    float s = 0.0f;
    if (c < C) {
#pragma unroll 8
        for (int64_t g = g0; g < g1; ++g) s = s + partials[g * THETA_STATS * D + c];
    }
    s_seg[seg][col] = s;
    __syncthreads();
    if (seg == 0 && c < C) {
        for (int k = 1; k < THETA_FINISH_SEGS; ++k) s = s + s_seg[k][col];
        grads[c] = s;
    }
}

inline bool misaligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) != 0; }

inline bool theta_shape_ok(int64_t N, int64_t S, int64_t R, int64_t D) {
    if (N < 0 || N > 0x7fffffff || D < 1 || D > THETA_MAX_D || S < 1) return false;
    return R == N || (R == S && N % S == 0);
}

template <bool VEC>
void theta_norm_launch(const ThetaNormArgs& a, dim3 grid, hipStream_t s) {
    const dim3 block(64 * THETA_WAVES);
    const int nu = ((VEC ? a.D / 4 : a.D) + 63) / 64;                   // units per lane: the smallest that holds it
#define THETA_FWD(NU) hipLaunchKernelGGL((theta_gamma_norm_kernel<NU, VEC>), grid, block, 0, s, a)
    if constexpr (VEC) {
        if (nu <= 1) THETA_FWD(1); else if (nu <= 2) THETA_FWD(2); else if (nu <= 3) THETA_FWD(3);
        else if (nu <= 4) THETA_FWD(4); else if (nu <= 6) THETA_FWD(6); else THETA_FWD(8);
    } else {
        if (nu <= 1) THETA_FWD(1); else if (nu <= 2) THETA_FWD(2); else if (nu <= 4) THETA_FWD(4);
        else if (nu <= 8) THETA_FWD(8); else if (nu <= 16) THETA_FWD(16); else THETA_FWD(32);
    }
#undef THETA_FWD
}

template <bool VEC, bool DERIV>
void theta_bwd_launch(const ThetaBwdArgs& a, dim3 grid, hipStream_t s) {
    const dim3 block(64 * THETA_WAVES);
    const int nu = ((VEC ? a.D / 4 : a.D) + 63) / 64;
#define THETA_BWD(NU) hipLaunchKernelGGL((theta_gamma_norm_backward_kernel<NU, VEC, DERIV>), grid, block, 0, s, a)
    if constexpr (VEC) {
        if (nu <= 1) THETA_BWD(1); else if (nu <= 2) THETA_BWD(2); else if (nu <= 3) THETA_BWD(3);
        else if (nu <= 4) THETA_BWD(4); else if (nu <= 6) THETA_BWD(6); else THETA_BWD(8);
    } else {
        if (nu <= 1) THETA_BWD(1); else if (nu <= 2) THETA_BWD(2); else if (nu <= 4) THETA_BWD(4);
        else if (nu <= 8) THETA_BWD(8); else if (nu <= 16) THETA_BWD(16); else THETA_BWD(32);
    }
#undef THETA_BWD
}

}  // namespace

extern "C" {

int aura_theta_gamma_table(const float* positions_or_null, int64_t start, int64_t R, int64_t D, const float* theta_off,
                           const float* gamma_off, const float* amp, int64_t max_seq_len, float ratio,
                           float* pe_or_null, float* d_theta_or_null, float* d_gamma_or_null, float* d_amp_or_null,
                           void* stream) {
    if (R < 0 || R > 0x7fffffff || D < 1 || D > THETA_MAX_D || max_seq_len < 1) return AURA_E_INVAL;
    if (!theta_off || !gamma_off || !amp) return AURA_E_INVAL;
    const int nd = (d_theta_or_null != nullptr) + (d_gamma_or_null != nullptr) + (d_amp_or_null != nullptr);
    if ((nd != 0 && nd != 3) || (nd == 0 && !pe_or_null)) return AURA_E_INVAL;
    if (misaligned(positions_or_null, 4) || misaligned(theta_off, 4) || misaligned(gamma_off, 4) ||
        misaligned(amp, 4) || misaligned(pe_or_null, 4) || misaligned(d_theta_or_null, 4) ||
        misaligned(d_gamma_or_null, 4) || misaligned(d_amp_or_null, 4))
        return AURA_E_ALIGN;
    if (R == 0) return AURA_OK;
    ThetaTableArgs a;
    a.pos = positions_or_null; a.th = theta_off; a.ga = gamma_off; a.amp = amp; a.pe = pe_or_null;
    a.d_th = d_theta_or_null; a.d_ga = d_gamma_or_null; a.d_amp = d_amp_or_null;
    a.start = start; a.R = R; a.D = (int)D;
    a.denom = (float)(max_seq_len - 1 > 1 ? max_seq_len - 1 : 1);
    a.ratio = ratio;
    const dim3 grid((unsigned)((R * D + 255) / 256)), block(256);
    hipLaunchKernelGGL(theta_gamma_table_kernel, grid, block, 0, static_cast<hipStream_t>(stream), a);
    return aura_check_launch();
}

int aura_theta_gamma_norm(const float* x, const float* table, const float* w, const float* b, float eps, int64_t N,
                          int64_t S, int64_t R, int64_t D, float* y, float* mean, float* rstd, void* stream) {
    if (!theta_shape_ok(N, S, R, D)) return AURA_E_INVAL;
    if (!x || !table || !w || !b || !y || !mean || !rstd) return AURA_E_INVAL;
    const uintptr_t al = D % 4 == 0 ? 16 : 4;
    if (misaligned(x, al) || misaligned(table, al) || misaligned(w, al) || misaligned(b, al) || misaligned(y, al) ||
        misaligned(mean, 4) || misaligned(rstd, 4))
        return AURA_E_ALIGN;
    if (N == 0) return AURA_OK;
    ThetaNormArgs a;
    a.x = x; a.table = table; a.w = w; a.b = b; a.y = y; a.mean = mean; a.rstd = rstd;
    a.N = N; a.S = S; a.D = (int)D; a.per_token = R == N; a.eps = eps;
    const dim3 grid((unsigned)((N + THETA_WAVES - 1) / THETA_WAVES));
    if (D % 4 == 0) theta_norm_launch<true>(a, grid, static_cast<hipStream_t>(stream));
    else theta_norm_launch<false>(a, grid, static_cast<hipStream_t>(stream));
    return aura_check_launch();
}

int64_t aura_theta_gamma_groups(int64_t N) { return N < 0 ? -1 : theta_groups(N); }

int aura_theta_gamma_norm_backward(const float* g_y, const float* x, const float* table, const float* d_theta_or_null,
                                   const float* d_gamma_or_null, const float* d_amp_or_null, const float* mean,
                                   const float* rstd, const float* w, int64_t N, int64_t S, int64_t R, int64_t D,
                                   float* g_x, float* partials_or_null, float* grads_or_null, void* stream) {
    if (!theta_shape_ok(N, S, R, D)) return AURA_E_INVAL;
    if (!g_y || !x || !table || !mean || !rstd || !w || !g_x) return AURA_E_INVAL;
    const int nd = (d_theta_or_null != nullptr) + (d_gamma_or_null != nullptr) + (d_amp_or_null != nullptr);
    if (nd != 0 && nd != 3) return AURA_E_INVAL;
    if ((partials_or_null == nullptr) != (grads_or_null == nullptr)) return AURA_E_INVAL;
    if (nd == 3 && !partials_or_null) return AURA_E_INVAL;
    const uintptr_t al = D % 4 == 0 ? 16 : 4;
    if (misaligned(g_y, al) || misaligned(x, al) || misaligned(table, al) || misaligned(d_theta_or_null, al) ||
        misaligned(d_gamma_or_null, al) || misaligned(d_amp_or_null, al) || misaligned(w, al) || misaligned(g_x, al) ||
        misaligned(partials_or_null, al) || misaligned(grads_or_null, 4) || misaligned(mean, 4) || misaligned(rstd, 4))
        return AURA_E_ALIGN;
    if (N == 0) return AURA_OK;
    const int64_t G = theta_groups(N);
    ThetaBwdArgs a;
    a.g_y = g_y; a.x = x; a.table = table; a.d_th = d_theta_or_null; a.d_ga = d_gamma_or_null; a.d_amp = d_amp_or_null;
    a.mean = mean; a.rstd = rstd; a.w = w; a.g_x = g_x; a.partials = partials_or_null;
    a.N = N; a.S = S; a.chunk = (N + G * THETA_WAVES - 1) / (G * THETA_WAVES);
    a.D = (int)D; a.per_token = R == N;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)G);
    const bool vec = D % 4 == 0;
    if (vec && nd) theta_bwd_launch<true, true>(a, grid, s);
    else if (vec) theta_bwd_launch<true, false>(a, grid, s);
    else if (nd) theta_bwd_launch<false, true>(a, grid, s);
    else theta_bwd_launch<false, false>(a, grid, s);
    if (partials_or_null) {
        const int C = (nd ? THETA_STATS : 2) * (int)D;
        hipLaunchKernelGGL(theta_gamma_finish_kernel, dim3((unsigned)((C + THETA_FINISH_COLS - 1) / THETA_FINISH_COLS)),
                           dim3(THETA_FINISH_COLS * THETA_FINISH_SEGS), 0, s, partials_or_null, grads_or_null, G, C,
                           (int)D);
    }
    return aura_check_launch();
}

}  // extern "C"
