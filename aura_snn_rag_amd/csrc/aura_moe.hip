// aura_moe.hip -- the MoE language zone: liquid routing, a device-side plan and sparse spiking experts (gfx950, wave64).
// The rule is stated once, in include/aura_hip.h ("MoE zone"); the comments here are about how it is computed.
//   route     a workgroup (4 waves) owns 32 consecutive rows, a wave eight of them, one after the other.  Lane l chains
//             the hidden units l, l + 64, .. of the row (the row itself sits in LDS), then lane e chains logit e, and the
//             softmax sum, the k rounds of the top-k and the renormalisation are wave reductions.  The workgroup counts
//             its (token, slot) pairs per expert in LDS and stores the E counts.
//   plan      one workgroup: per expert an exclusive scan of the route workgroups' counts (so a pair's place is its
//             expert's base + its workgroup's offset + its rank inside the workgroup: no atomic decides a place), the
//             experts' bases and the table of tiles: at most 32 pairs of one expert each.
//   scatter   the route workgroups again, one thread per pair: the rank is the number of earlier rows of the workgroup
//             with the same expert, counted from LDS.  pairs[place] = token k + slot.
//   experts   one workgroup per tile; the grid is the bound ceil(P / 32) + E and a workgroup beyond the table leaves.
//             The 32 rows are gathered into LDS; every linear is C[32 x 32] blocks of v_mfma_f32_32x32x2_f32 with the
//             activations (LDS) as the row operand and the weights (global, through the pointer table, 16 bytes per
//             lane along k) as the column operand, a wave per block of 32 outputs.  The GIF step is the epilogue of a
//             layer's second linear; two LDS buffers take turns as input and output.
//   combine   one thread per four outputs of a token: the token's slots in ascending expert id.
// Five launches, no global atomics, no host read.  A row of the MFMA's row operand touches no other row's result, so a
// token's bits do not depend on its tile.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/aura_hip.h"
#include "aura_common.inl"

namespace {

#include "aura_gif_model.inl"

constexpr int MOE_ROWS = 32;            // rows of a route workgroup and pairs of a tile
constexpr int MOE_MAX_DM = AURA_MOE_MAX_DM, MOE_MAX_HR = AURA_MOE_MAX_HR, MOE_MAX_E = AURA_MOE_MAX_E;
constexpr int MOE_MAX_K = AURA_MOE_MAX_K;

inline int64_t moe_groups(int64_t N) { return (N + MOE_ROWS - 1) / MOE_ROWS; }
inline int64_t moe_max_tiles(int64_t N, int64_t E, int64_t k) { return (N * k + MOE_ROWS - 1) / MOE_ROWS + E; }

// the workspace, all int32: counts [G][E], offs [G][E], base [E] + n_tiles [1], tiles [max_tiles][3], pairs [P]
struct MoeWorkspace {
    int *counts, *offs, *base, *n_tiles, *tiles, *pairs;
    int64_t bytes;
};
inline MoeWorkspace moe_workspace(void* ws, int64_t N, int64_t E, int64_t k) {
    const int64_t G = moe_groups(N);
    const int64_t a = aura_align256(G * E * 4), b = aura_align256((E + 1) * 4), c = aura_align256(moe_max_tiles(N, E, k) * 12),
                  d = aura_align256(N * k * 4);
    char* p = static_cast<char*>(ws);
    MoeWorkspace w;
    w.counts = reinterpret_cast<int*>(p);
    w.offs = reinterpret_cast<int*>(p + a);
    w.base = reinterpret_cast<int*>(p + 2 * a);
    w.n_tiles = w.base + E;
    w.tiles = reinterpret_cast<int*>(p + 2 * a + b);
    w.pairs = reinterpret_cast<int*>(p + 2 * a + b + c);
    w.bytes = 2 * a + b + c + d;
    return w;
}

struct MoeRouteArgs {
    const float *x, *U, *bU, *bW, *gate_w, *gate_b, *attn_gain;
    int* indices;
    float *weights, *probs;
    int* counts;
    float dt, temperature;
    int64_t N;
    int Dm, Hr, E, k;
};

// LDS written by one lane of a wave is read by another: order the accesses within the wave
__device__ __forceinline__ void wave_sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

__global__ __launch_bounds__(256) void moe_route_kernel(const MoeRouteArgs a) {
    __shared__ float4 s_x[4][MOE_MAX_DM / 4];
    __shared__ float4 s_h[4][MOE_MAX_HR / 4];
    __shared__ int s_hist[MOE_MAX_E];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Dm = a.Dm, Hr = a.Hr, E = a.E, k = a.k;
    if (tid < MOE_MAX_E) s_hist[tid] = 0;
    __syncthreads();
    float* const hs = reinterpret_cast<float*>(s_h[wave]);
    const int64_t row0 = (int64_t)blockIdx.x * MOE_ROWS + wave * 8;
    for (int i = 0; i < 8; ++i) {
        const int64_t row = row0 + i;
        if (row >= a.N) break;                                           // uniform over the wave
        for (int c = lane; c < Dm / 4; c += 64) s_x[wave][c] = reinterpret_cast<const float4*>(a.x)[row * (Dm / 4) + c];
        wave_sync_lds();
        // 1, 2: h = fl(dt tanhf(fl(bW + fl(dot + bU))))
        for (int j = lane; j < Hr; j += 64) {
            const float4* const u = reinterpret_cast<const float4*>(a.U + (int64_t)j * Dm);
            float t = 0.0f;
            for (int c = 0; c < Dm / 4; ++c) {
                const float4 w = u[c], v = s_x[wave][c];
                t = fmaf(w.x, v.x, t); t = fmaf(w.y, v.y, t); t = fmaf(w.z, v.z, t); t = fmaf(w.w, v.w, t);
            }
            const float pre = a.bW[j] + (t + a.bU[j]);
            hs[j] = a.dt * tanhf(pre);
        }
        wave_sync_lds();
        // 3, 4: the logit of expert `lane`
        const bool live = lane < E;
        float z = 0.0f;
        if (live) {
            const float* const g = a.gate_w + (int64_t)lane * Hr;
            float t = 0.0f;
            for (int j = 0; j < Hr; ++j) t = fmaf(g[j], hs[j], t);
            z = t + a.gate_b[lane];
            float temp = a.temperature;
            if (a.attn_gain) temp = fminf(fmaxf(a.temperature / (a.attn_gain[row] + 1e-6f), 0.1f), 5.0f);
            z = z / temp;
        }
        // 5: softmax; lanes beyond E add +0 to the butterfly
        float mx = live ? z : -INFINITY;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m, 64));
        const float ex = live ? expf(z - mx) : 0.0f;
        const float p = ex / wave_sum(ex);
        if (live) a.probs[row * E + lane] = p;
        // 6: k rounds of (value descending, id ascending), NaN first: the largest 64-bit key, -1 = taken or no expert
        long long key = -1;
        if (live) {
            const uint32_t bits = (p != p) ? 0x7fffffffu : (__float_as_uint(p) & 0x7fffffffu);
            key = ((long long)bits << 32) | (long long)(63 - lane);
        }
        float total = 0.0f, mine = 0.0f;
        int my_e = 0;
        for (int r = 0; r < k; ++r) {
            long long best = key;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const long long o = __shfl_xor(best, m, 64);
                best = o > best ? o : best;
            }
            const int e = 63 - (int)(best & 63);
            const float pe = __shfl(p, e, 64);
            total = r == 0 ? pe : total + pe;                            // 7: the sum in rank order
            if (lane == e) key = -1;
            if (lane == r) { mine = pe; my_e = e; }
        }
        if (lane < k) {
            a.indices[row * k + lane] = my_e;
            a.weights[row * k + lane] = mine / (total + 1e-8f);
            atomicAdd(&s_hist[my_e], 1);                                 // LDS: a count, never a place
        }
        wave_sync_lds();
    }
    __syncthreads();
    if (tid < E) a.counts[(int64_t)blockIdx.x * E + tid] = s_hist[tid];
}

// One workgroup.  offs[g][e] = pairs of expert e in the route workgroups before g; base[e]; the tile table.
__global__ __launch_bounds__(256) void moe_plan_kernel(const int* __restrict__ counts, int* __restrict__ offs,
                                                       int* __restrict__ base, int* __restrict__ n_tiles,
                                                       int* __restrict__ tiles, int G, int E) {
    __shared__ int s_wave[4];
    __shared__ int s_cnt[MOE_MAX_E], s_base[MOE_MAX_E + 1], s_tile0[MOE_MAX_E + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int e = 0; e < E; ++e) {
        int running = 0;
        for (int g0 = 0; g0 < G; g0 += 256) {
            const int g = g0 + tid;
            const int v = g < G ? counts[(int64_t)g * E + e] : 0;
            int inc = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_up(inc, d, 64);
                if (lane >= d) inc += o;
            }
            if (lane == 63) s_wave[wave] = inc;
            __syncthreads();
            int before = 0, all = 0;
            for (int w = 0; w < 4; ++w) {
                if (w < wave) before += s_wave[w];
                all += s_wave[w];
            }
            if (g < G) offs[(int64_t)g * E + e] = running + before + inc - v;
            running += all;
            __syncthreads();
        }
        if (tid == 0) s_cnt[e] = running;
    }
    __syncthreads();
    if (tid == 0) {
        int b = 0, t = 0;
        for (int e = 0; e < E; ++e) {
            s_base[e] = b; s_tile0[e] = t;
            base[e] = b;
            b += s_cnt[e];
            t += (s_cnt[e] + MOE_ROWS - 1) / MOE_ROWS;
        }
        s_base[E] = b; s_tile0[E] = t;
        *n_tiles = t;
    }
    __syncthreads();
    const int T = s_tile0[E];
    for (int t = tid; t < T; t += 256) {
        int e = 0;
        while (s_tile0[e + 1] <= t) ++e;                                 // terminates: t < s_tile0[E]
        const int first = (t - s_tile0[e]) * MOE_ROWS;
        const int left = s_cnt[e] - first;
        tiles[3 * t] = e;
        tiles[3 * t + 1] = s_base[e] + first;
        tiles[3 * t + 2] = left < MOE_ROWS ? left : MOE_ROWS;
    }
}

// The route workgroups again: thread (row, slot) of the 32 rows finds its pair's place.
__global__ __launch_bounds__(256) void moe_scatter_kernel(const int* __restrict__ indices, const int* __restrict__ offs,
                                                          const int* __restrict__ base, int* __restrict__ pairs,
                                                          int64_t N, int E, int k) {
    __shared__ int s_e[MOE_ROWS * MOE_MAX_K];
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * MOE_ROWS;
    const int64_t rows = N - row0 < MOE_ROWS ? N - row0 : MOE_ROWS;
    const int n = (int)rows * k;
    if (tid < n) s_e[tid] = indices[row0 * k + tid];
    __syncthreads();
    if (tid >= n) return;
    const int e = s_e[tid], r = tid / k;
    int rank = 0;
    for (int j = 0; j < r * k; ++j) rank += s_e[j] == e ? 1 : 0;
    pairs[base[e] + offs[(int64_t)blockIdx.x * E + e] + rank] = (int)(row0 * k) + tid;
}

struct MoeExpertArgs {
    const float* x;
    const float* const* ptrs;           // [E][4 layers + 2]: per layer W_s, b_s, W_g, b_g; then W_r, b_r
    const float* gif;                   // [E][layers][4]: decay, L, alpha, threshold
    const int *tiles, *n_tiles, *pairs;
    float *y, *trace;
    int Dm, Hh, layers, k, stride;
};

// One linear of the chain over the tile's 32 rows: out[row][n] = fl(dot_K(in[row], W[n]) + b[n]), handed to `epi`.  The
// dot is the MFMA chain: per 8 consecutive k, the pairs (k, k + 4), (k + 1, k + 5), .. in this order, each pair in
// ascending k, from 0; a k beyond K enters as 0 x 0.
template <class Epi>
__device__ __forceinline__ void moe_linear(const float* in, int stride, int K, const float* __restrict__ W,
                                           const float* __restrict__ b, int Nout, Epi epi) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float* const arow = in + l31 * stride;
    for (int nb = wave; nb * 32 < Nout; nb += 4) {
        const int n = nb * 32 + l31;
        const bool n_ok = n < Nout;
        const float* const wrow = W + (int64_t)(n_ok ? n : 0) * K;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll 4
        for (int k0 = 0; k0 < K; k0 += 8) {
            const int kk = k0 + 4 * half;
            const bool ok = kk < K;
            const float4 av = *reinterpret_cast<const float4*>(arow + (ok ? kk : 0));
            const float4 wv = *reinterpret_cast<const float4*>(wrow + (ok ? kk : 0));
            acc = aura_mfma_f32_x4(ok ? av : zero, (ok && n_ok) ? wv : zero, acc);
        }
        if (n_ok) {
            const float bias = b[n];
#pragma unroll
            for (int r = 0; r < 16; ++r) epi((r & 3) + 8 * (r >> 2) + 4 * half, n, acc[r] + bias);
        }
    }
}

__global__ __launch_bounds__(256) void moe_experts_kernel(const MoeExpertArgs a) {
    extern __shared__ float4 s_dyn[];
    __shared__ int s_pair[MOE_ROWS];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= *a.n_tiles) return;
    const int e = a.tiles[3 * blockIdx.x], begin = a.tiles[3 * blockIdx.x + 1], cnt = a.tiles[3 * blockIdx.x + 2];
    const int Dm = a.Dm, Hh = a.Hh, L = a.layers, stride = a.stride;
    float* bufA = reinterpret_cast<float*>(s_dyn);
    float* bufB = bufA + MOE_ROWS * stride;
    if (tid < MOE_ROWS) s_pair[tid] = tid < cnt ? a.pairs[begin + tid] : -1;
    __syncthreads();
    const int q = Dm / 4;
    for (int i = tid; i < MOE_ROWS * q; i += 256) {
        const int row = i / q, c = i - row * q, pair = s_pair[row];
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (pair >= 0) v = reinterpret_cast<const float4*>(a.x)[(int64_t)(pair / a.k) * q + c];
        *reinterpret_cast<float4*>(bufA + row * stride + 4 * c) = v;
    }
    __syncthreads();
    const float* const* const P = a.ptrs + (int64_t)e * (4 * L + 2);
    for (int l = 0; l < L; ++l) {
        const float* const gp = a.gif + ((int64_t)e * L + l) * 4;
        GifModel<false> gm;
        gm.decay = gp[0]; gm.Lf = gp[1]; gm.alpha = gp[2]; gm.thr0 = gp[3];
        moe_linear(bufA, stride, l == 0 ? Dm : Hh, P[4 * l], P[4 * l + 1], Hh,
                   [&](int row, int n, float v) { bufB[row * stride + n] = v; });
        __syncthreads();
        moe_linear(bufB, stride, Hh, P[4 * l + 2], P[4 * l + 3], Hh, [&](int row, int n, float v) {
            GifModel<false>::Lane ln{0.0f, gm.thr0};
            const float s = gm.step(ln, v);
            bufA[row * stride + n] = s;
            const int pair = s_pair[row];
            if (a.trace && pair >= 0) a.trace[((int64_t)pair * L + l) * Hh + n] = s;
        });
        __syncthreads();
    }
    moe_linear(bufA, stride, Hh, P[4 * L], P[4 * L + 1], Dm, [&](int row, int n, float v) {
        const int pair = s_pair[row];
        if (pair >= 0) a.y[(int64_t)pair * Dm + n] = v;
    });
}

// out[token][d] = sum of fl(w_j y_j[d]) over the token's slots in ascending expert id, from the first product.
__global__ __launch_bounds__(256) void moe_combine_kernel(const int* __restrict__ indices, const float* __restrict__ weights,
                                                          const float* __restrict__ y, float* __restrict__ out,
                                                          int64_t N, int q, int k) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N * q) return;
    const int64_t token = i / q;
    const int c = (int)(i - token * q);
    const int* const idx = indices + token * k;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int last = -1;
    for (int r = 0; r < k; ++r) {
        int best = 0x7fffffff, slot = 0;
        for (int j = 0; j < k; ++j) {                                     // the smallest id above the last one taken
            const int ej = idx[j];
            if (ej > last && ej < best) { best = ej; slot = j; }
        }
        last = best;
        const float w = weights[token * k + slot];
        const float4 v = reinterpret_cast<const float4*>(y)[(token * k + slot) * q + c];
        const float4 p = make_float4(w * v.x, w * v.y, w * v.z, w * v.w);
        if (r == 0) acc = p;
        else { acc.x = acc.x + p.x; acc.y = acc.y + p.y; acc.z = acc.z + p.z; acc.w = acc.w + p.w; }
    }
    reinterpret_cast<float4*>(out)[i] = acc;
}

inline bool misaligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) != 0; }

inline bool moe_counts_ok(int64_t N, int64_t E, int64_t k) {
    return N >= 0 && N <= AURA_MOE_MAX_N && E >= 1 && E <= MOE_MAX_E && k >= 1 && k <= MOE_MAX_K && k <= E;
}

}  // namespace

extern "C" {

int64_t aura_moe_workspace_bytes(int64_t N, int64_t E, int64_t k) {
    if (!moe_counts_ok(N, E, k)) return -1;
    return moe_workspace(nullptr, N, E, k).bytes;
}

int aura_moe_route(const float* x, int64_t N, int64_t Dm, const float* U, const float* bU, const float* bW, int64_t Hr,
                   float dt, const float* gate_w, const float* gate_b, int64_t E, int64_t k, float temperature,
                   const float* attn_gain_or_null, int32_t* indices, float* weights, float* probs, void* workspace,
                   int64_t workspace_bytes, void* stream) {
    if (!moe_counts_ok(N, E, k)) return AURA_E_INVAL;
    if (Dm % 4 || Dm < 4 || Dm > MOE_MAX_DM || Hr < 1 || Hr > MOE_MAX_HR) return AURA_E_INVAL;
    if (!x || !U || !bU || !bW || !gate_w || !gate_b || !indices || !weights || !probs || !workspace) return AURA_E_INVAL;
    if (workspace_bytes < aura_moe_workspace_bytes(N, E, k)) return AURA_E_INVAL;
    if (misaligned(x, 16) || misaligned(U, 16) || misaligned(workspace, 256) || misaligned(bU, 4) || misaligned(bW, 4) ||
        misaligned(gate_w, 4) || misaligned(gate_b, 4) || misaligned(attn_gain_or_null, 4) || misaligned(indices, 4) ||
        misaligned(weights, 4) || misaligned(probs, 4))
        return AURA_E_ALIGN;
    if (N == 0) return AURA_OK;
    const MoeWorkspace w = moe_workspace(workspace, N, E, k);
    MoeRouteArgs a;
    a.x = x; a.U = U; a.bU = bU; a.bW = bW; a.gate_w = gate_w; a.gate_b = gate_b; a.attn_gain = attn_gain_or_null;
    a.indices = indices; a.weights = weights; a.probs = probs; a.counts = w.counts;
    a.dt = dt; a.temperature = temperature; a.N = N;
    a.Dm = (int)Dm; a.Hr = (int)Hr; a.E = (int)E; a.k = (int)k;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int G = (int)moe_groups(N);
    hipLaunchKernelGGL(moe_route_kernel, dim3(G), dim3(256), 0, s, a);
    if (aura_check_launch() != AURA_OK) return AURA_E_LAUNCH;
    hipLaunchKernelGGL(moe_plan_kernel, dim3(1), dim3(256), 0, s, w.counts, w.offs, w.base, w.n_tiles, w.tiles, G, (int)E);
    if (aura_check_launch() != AURA_OK) return AURA_E_LAUNCH;
    hipLaunchKernelGGL(moe_scatter_kernel, dim3(G), dim3(256), 0, s, indices, w.offs, w.base, w.pairs, N, (int)E, (int)k);
    return aura_check_launch();
}

int aura_moe_experts(const float* x, int64_t N, int64_t Dm, int64_t Hh, int64_t layers, int64_t E, int64_t k,
                     const void* ptr_table, const float* gif_table, const int32_t* indices, const float* weights,
                     float* y, float* out, float* trace_or_null, const void* workspace, int64_t workspace_bytes,
                     void* stream) {
    if (!moe_counts_ok(N, E, k)) return AURA_E_INVAL;
    if (Dm % 4 || Dm < 4 || Dm > MOE_MAX_DM || Hh % 4 || Hh < 4 || Hh > AURA_MOE_MAX_HH) return AURA_E_INVAL;
    if (layers < 1 || layers > AURA_MOE_MAX_LAYERS) return AURA_E_INVAL;
    if (!x || !ptr_table || !gif_table || !indices || !weights || !y || !out || !workspace) return AURA_E_INVAL;
    if (workspace_bytes < aura_moe_workspace_bytes(N, E, k)) return AURA_E_INVAL;
    if (misaligned(x, 16) || misaligned(y, 16) || misaligned(out, 16) || misaligned(workspace, 256) ||
        misaligned(ptr_table, 8) || misaligned(gif_table, 4) || misaligned(indices, 4) || misaligned(weights, 4) ||
        misaligned(trace_or_null, 4))
        return AURA_E_ALIGN;
    if (N == 0) return AURA_OK;
    const MoeWorkspace w = moe_workspace(const_cast<void*>(workspace), N, E, k);
    MoeExpertArgs a;
    a.x = x; a.ptrs = static_cast<const float* const*>(ptr_table); a.gif = gif_table;
    a.tiles = w.tiles; a.n_tiles = w.n_tiles; a.pairs = w.pairs; a.y = y; a.trace = trace_or_null;
    a.Dm = (int)Dm; a.Hh = (int)Hh; a.layers = (int)layers; a.k = (int)k;
    const int kmax = (int)(Dm > Hh ? Dm : Hh);
    a.stride = kmax + 4;                                                 // a multiple of 4: rows stay 16-byte aligned
    const int lds = 2 * MOE_ROWS * a.stride * (int)sizeof(float);        // at most 132096 bytes (Hh = 512)
    if (aura_ensure_lds_attr(reinterpret_cast<const void*>(moe_experts_kernel), 2 * MOE_ROWS * (AURA_MOE_MAX_HH + 4) * 4))
        return AURA_E_LAUNCH;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(moe_experts_kernel, dim3((unsigned)moe_max_tiles(N, E, k)), dim3(256), lds, s, a);
    if (aura_check_launch() != AURA_OK) return AURA_E_LAUNCH;
    const int64_t n4 = N * (Dm / 4);
    hipLaunchKernelGGL(moe_combine_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, indices, weights, y, out,
                       N, (int)(Dm / 4), (int)k);
    return aura_check_launch();
}

}  // extern "C"
