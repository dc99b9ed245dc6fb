// aura_place.hip -- the place-cell code: exact k-winner selection, sigmoid, sparse reconstruction and the dense code in
// one launch; the logit gradient in a mirror launch (gfx950).
// The rule is stated once, in include/aura_hip.h ("Place code"); the comments here are about how it is computed.
//   rows       one wave owns a row from its logits to its outputs; a workgroup is four waves = four rows that share
//              nothing, so there is no workgroup barrier and a wave beyond the last row simply leaves.
//   keys       the row sits in registers as EPT monotone keys per lane (cell = 64 j + lane): the float's bits with the
//              sign folded so that unsigned order is value order, -0 as +0, every NaN as the largest key.  A cell beyond
//              P holds key 0, below every real key (-inf is 0x007fffff).
//   selection  the k-th largest key T by bisection, bit 31 down to 0: "do at least k keys reach T | bit?", counted by
//              one compare and one ballot per register (the popcounts and the sum are scalar work).  Keys above T win;
//              of the keys equal to T the first k - #(above) in cell order win.
//   compaction a running ballot prefix over j ascending gives every winner its position in ascending cell order; the
//              winners' cells and logits go to the wave's LDS list, then lane r turns logit r into its activation
//              (ceil(k / 64) expf per lane instead of one per register) and writes idx / act coalesced.
//   dense row  place_write_row: per 64 cells, the winners that fall there (a contiguous run of the sorted list, found by
//              ballots over the list held in registers) are dropped through a 64-float LDS window into their lanes; one
//              coalesced store per 64 cells, every element written once.
//   gather     out: per tile of 1024 (256 without float4) outputs the wave walks its k winners in list order; the row
//              index and activation are wave-uniform (readfirstlane), the table row is read 16 bytes per lane.
//   LDS        per wave 256 cells + 256 values + the 64-float window = 2304 bytes.  A wave's LDS operations execute in
//              program order, so the list written by some lanes is read by others after a compiler fence only.
// No atomics anywhere; nothing depends on N, on the grid or on the device.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/aura_hip.h"
#include "aura_common.inl"

namespace {

constexpr int PLACE_WAVES = 4;          // rows per workgroup
constexpr int PLACE_MAX_K = 256;
constexpr int PLACE_SLOTS = PLACE_MAX_K / 64;
constexpr int PLACE_MAX_P = 8192;
constexpr int PLACE_CHUNKS = 4;         // 64-lane chunks of outputs a wave carries through one walk of its winners

struct PlaceArgs {
    const float* z;                     // [N][P]
    const float* e;                     // [N][D]
    const float* W2t;                   // [P][D]
    const float* b2;                    // [D]
    int32_t* idx;                       // [N][k]
    float* act;                         // [N][k]
    float* out;                         // [N][D]
    float* dense;                       // [N][P] or NULL
    int64_t N;
    int P, D, k;
};

struct PlaceBwdArgs {
    const float* g_out;                 // [N][D]
    const float* g_dense;               // [N][P] or NULL
    const int32_t* idx;                 // [N][k]
    const float* act;                   // [N][k]
    const float* W2t;                   // [P][D]
    float* g_z;                         // [N][P]
    int64_t N;
    int P, D, k;
};

__device__ __forceinline__ uint32_t place_key(float z) {
    uint32_t u = __float_as_uint(z);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;            // NaN: above +inf, all equal
    if (u == 0x80000000u) u = 0u;                                        // -0 is +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// the logit of a key (a NaN comes back as some NaN, -0 as +0: neither changes the activation)
__device__ __forceinline__ float place_unkey(uint32_t key) {
    return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}
__device__ __forceinline__ uint64_t place_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ int place_count(uint64_t m) { return __builtin_popcountll(m); }
// how many lanes below this one are set in m
__device__ __forceinline__ int place_prefix(uint64_t m) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// the wave's LDS list written by some lanes is read by others: program order is enough for the hardware, this keeps the
// compiler to it
__device__ __forceinline__ void place_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ int place_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float place_uniform(float v) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

// One dense row [P]: +0.0 everywhere except s_val[r] at cell s_idx[r], r < k, the list ascending in cell.
__device__ __forceinline__ void place_write_row(const int* s_idx, const float* s_val, float* s_row, int k, int P,
                                                float* row_out, int lane) {
    int widx[PLACE_SLOTS];
#pragma unroll
    for (int s = 0; s < PLACE_SLOTS; ++s) {
        const int r = s * 64 + lane;
        widx[s] = r < k ? s_idx[r] : 0x7fffffff;
    }
    int lo = 0;
    for (int c0 = 0; c0 < P; c0 += 64) {
        int hi = 0;                                                      // winners below cell c0 + 64
#pragma unroll
        for (int s = 0; s < PLACE_SLOTS; ++s)
            if (s * 64 < k) hi += place_count(place_ballot(widx[s] < c0 + 64));
        float v = 0.0f;
        if (hi > lo) {                                                   // uniform over the wave
            s_row[lane] = 0.0f;
            place_wave_sync();
            if (lane < hi - lo) s_row[s_idx[lo + lane] & 63] = s_val[lo + lane];
            place_wave_sync();
            v = s_row[lane];
            place_wave_sync();
        }
        if (c0 + lane < P) row_out[c0 + lane] = v;
        lo = hi;
    }
}

// VEC: D % 4 == 0 and 16-byte aligned rows.  A unit is a float4 (VEC) or a float; U = units per row.
template <bool VEC> struct PlaceUnit;
template <> struct PlaceUnit<true> {
    typedef float4 T;
    static __device__ __forceinline__ T zero() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
    static __device__ __forceinline__ T fma(float a, T w, T c) {
        return make_float4(fmaf(a, w.x, c.x), fmaf(a, w.y, c.y), fmaf(a, w.z, c.z), fmaf(a, w.w, c.w));
    }
    static __device__ __forceinline__ T finish(T e, T acc, T b) {
        return make_float4(e.x + 0.1f * (acc.x + b.x), e.y + 0.1f * (acc.y + b.y), e.z + 0.1f * (acc.z + b.z),
                           e.w + 0.1f * (acc.w + b.w));
    }
    static __device__ __forceinline__ float dot(T g, T w, float p) {
        return fmaf(g.w, w.w, fmaf(g.z, w.z, fmaf(g.y, w.y, fmaf(g.x, w.x, p))));
    }
};
template <> struct PlaceUnit<false> {
    typedef float T;
    static __device__ __forceinline__ T zero() { return 0.0f; }
    static __device__ __forceinline__ T fma(float a, T w, T c) { return fmaf(a, w, c); }
    static __device__ __forceinline__ T finish(T e, T acc, T b) { return e + 0.1f * (acc + b); }
    static __device__ __forceinline__ float dot(T g, T w, float p) { return fmaf(g, w, p); }
};

template <int EPT, bool VEC>
__global__ __launch_bounds__(64 * PLACE_WAVES) void place_code_kernel(const PlaceArgs a) {
    __shared__ int s_idx_all[PLACE_WAVES][PLACE_MAX_K];
    __shared__ float s_val_all[PLACE_WAVES][PLACE_MAX_K];
    __shared__ float s_row_all[PLACE_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n = (int64_t)blockIdx.x * PLACE_WAVES + wave;
    if (n >= a.N) return;
    int* const s_idx = s_idx_all[wave];
    float* const s_val = s_val_all[wave];
    const int P = a.P, D = a.D, k = a.k;

    // ---- the row as keys
    const float* const zr = a.z + n * P;
    uint32_t key[EPT];
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int c = j * 64 + lane;
        key[j] = c < P ? place_key(zr[c]) : 0u;
    }

    // ---- T = the k-th largest key
    uint32_t T = 0u;
#pragma unroll 1
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t cand = T | (1u << bit);
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < EPT; ++j) cnt += place_count(place_ballot(key[j] >= cand));
        if (cnt >= k) T = cand;
    }
    int above = 0;
#pragma unroll
    for (int j = 0; j < EPT; ++j) above += place_count(place_ballot(key[j] > T));
    const int need = k - above;                                          // of the keys equal to T, in cell order

    // ---- winners to the list, ascending cell
    int eq_base = 0, w_base = 0;
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const bool is_eq = key[j] == T;
        const uint64_t beq = place_ballot(is_eq);
        const bool win = key[j] > T || (is_eq && eq_base + place_prefix(beq) < need);
        const uint64_t bw = place_ballot(win);
        if (win) {
            const int pos = w_base + place_prefix(bw);                   // < k: exactly k cells win
            s_idx[pos] = j * 64 + lane;
            s_val[pos] = place_unkey(key[j]);
        }
        eq_base += place_count(beq);
        w_base += place_count(bw);
    }
    place_wave_sync();

    // ---- activations; idx and act leave coalesced
#pragma unroll
    for (int s = 0; s < PLACE_SLOTS; ++s) {
        const int r = s * 64 + lane;
        if (r < k) {
            const float act = 1.0f / (1.0f + expf(-s_val[r]));
            s_val[r] = act;
            a.idx[n * k + r] = s_idx[r];
            a.act[n * k + r] = act;
        }
    }
    place_wave_sync();

    if (a.dense) place_write_row(s_idx, s_val, s_row_all[wave], k, P, a.dense + n * P, lane);

    // ---- out = e + 0.1 (sum_j act_j W2t[j] + b2), the winners in list order
    typedef PlaceUnit<VEC> UT;
    typedef typename UT::T unit;
    const int U = VEC ? D / 4 : D;
    const unit* const er = reinterpret_cast<const unit*>(a.e + n * D);
    const unit* const b2 = reinterpret_cast<const unit*>(a.b2);
    unit* const outr = reinterpret_cast<unit*>(a.out + n * D);
    for (int u0 = 0; u0 < U; u0 += 64 * PLACE_CHUNKS) {
        unit acc[PLACE_CHUNKS];
        int q[PLACE_CHUNKS];
#pragma unroll
        for (int c = 0; c < PLACE_CHUNKS; ++c) {
            acc[c] = UT::zero();
            const int u = u0 + c * 64 + lane;
            q[c] = u < U ? u : U - 1;                                    // every lane loads: a lane beyond the row
        }                                                                // re-reads its last unit and stores nothing
        for (int j = 0; j < k; ++j) {
            const int row = place_uniform(s_idx[j]);
            const float aj = place_uniform(s_val[j]);
            const unit* const w = reinterpret_cast<const unit*>(a.W2t + (int64_t)row * D);
#pragma unroll
            for (int c = 0; c < PLACE_CHUNKS; ++c)
                if (u0 + c * 64 < U) acc[c] = UT::fma(aj, w[q[c]], acc[c]);   // uniform over the wave
        }
#pragma unroll
        for (int c = 0; c < PLACE_CHUNKS; ++c)
            if (u0 + c * 64 + lane < U) outr[q[c]] = UT::finish(er[q[c]], acc[c], b2[q[c]]);
    }
}

template <bool VEC>
__global__ __launch_bounds__(64 * PLACE_WAVES) void place_code_backward_kernel(const PlaceBwdArgs a) {
    __shared__ int s_idx_all[PLACE_WAVES][PLACE_MAX_K];
    __shared__ float s_val_all[PLACE_WAVES][PLACE_MAX_K];
    __shared__ float s_row_all[PLACE_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n = (int64_t)blockIdx.x * PLACE_WAVES + wave;
    if (n >= a.N) return;
    int* const s_idx = s_idx_all[wave];
    float* const s_val = s_val_all[wave];
    const int P = a.P, D = a.D, k = a.k;

#pragma unroll
    for (int s = 0; s < PLACE_SLOTS; ++s) {
        const int r = s * 64 + lane;
        if (r < k) {
            s_idx[r] = a.idx[n * k + r];
            s_val[r] = a.act[n * k + r];
        }
    }
    place_wave_sync();

    // ---- tot[s] of lane l = <g_out[n], W2t[idx[64 s + l]]>
    typedef PlaceUnit<VEC> UT;
    typedef typename UT::T unit;
    const int U = VEC ? D / 4 : D;
    const unit* const gr = reinterpret_cast<const unit*>(a.g_out + n * D);
    float tot[PLACE_SLOTS];
#pragma unroll
    for (int s = 0; s < PLACE_SLOTS; ++s) tot[s] = 0.0f;
    for (int u0 = 0; u0 < U; u0 += 64 * PLACE_CHUNKS) {
        unit g[PLACE_CHUNKS];
        int q[PLACE_CHUNKS];
        bool live[PLACE_CHUNKS];
#pragma unroll
        for (int c = 0; c < PLACE_CHUNKS; ++c) {
            const int u = u0 + c * 64 + lane;
            live[c] = u < U;
            q[c] = live[c] ? u : U - 1;
            g[c] = gr[q[c]];
        }
#pragma unroll
        for (int s = 0; s < PLACE_SLOTS; ++s) {
            const int ks = k - s * 64 < 64 ? k - s * 64 : 64;            // winners of this slot (may be <= 0)
            for (int jj = 0; jj < ks; ++jj) {
                int row = place_uniform(s_idx[s * 64 + jj]);
                row = row < 0 ? 0 : (row >= P ? P - 1 : row);
                const unit* const w = reinterpret_cast<const unit*>(a.W2t + (int64_t)row * D);
                float p = 0.0f;
#pragma unroll
                for (int c = 0; c < PLACE_CHUNKS; ++c)
                    if (u0 + c * 64 < U) {                               // uniform over the wave
                        const float pc = UT::dot(g[c], w[q[c]], p);
                        p = live[c] ? pc : p;
                    }
                p = p + __shfl_xor(p, 32);
                p = p + __shfl_xor(p, 16);
                p = p + __shfl_xor(p, 8);
                p = p + __shfl_xor(p, 4);
                p = p + __shfl_xor(p, 2);
                p = p + __shfl_xor(p, 1);
                if (lane == jj) tot[s] = tot[s] + p;
            }
        }
    }

    // ---- g_z at the winners, then the whole row
#pragma unroll
    for (int s = 0; s < PLACE_SLOTS; ++s) {
        const int r = s * 64 + lane;
        if (r < k) {
            const float act = s_val[r];
            float g_act = 0.1f * tot[s];
            if (a.g_dense) {
                int cell = s_idx[r];
                cell = cell < 0 ? 0 : (cell >= P ? P - 1 : cell);
                g_act = g_act + a.g_dense[n * P + cell];
            }
            s_val[r] = (g_act * act) * (1.0f - act);
        }
    }
    place_wave_sync();
    place_write_row(s_idx, s_val, s_row_all[wave], k, P, a.g_z + n * P, lane);
}

inline bool place_shape_ok(int64_t N, int64_t P, int64_t D, int64_t k) {
    return N >= 0 && N <= 0x7fffffff && P >= 1 && P <= PLACE_MAX_P && D >= 1 && D <= 0x7fffffff && k >= 1 &&
           k <= PLACE_MAX_K && k <= P;
}
inline bool misaligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) != 0; }

template <bool VEC>
void place_launch(const PlaceArgs& a, dim3 grid, hipStream_t s) {
    const dim3 block(64 * PLACE_WAVES);
    // registers per lane for a row of P cells: the smallest of these that holds it
    if (a.P <= 64) hipLaunchKernelGGL((place_code_kernel<1, VEC>), grid, block, 0, s, a);
    else if (a.P <= 128) hipLaunchKernelGGL((place_code_kernel<2, VEC>), grid, block, 0, s, a);
    else if (a.P <= 512) hipLaunchKernelGGL((place_code_kernel<8, VEC>), grid, block, 0, s, a);
    else if (a.P <= 1024) hipLaunchKernelGGL((place_code_kernel<16, VEC>), grid, block, 0, s, a);
    else if (a.P <= 2048) hipLaunchKernelGGL((place_code_kernel<32, VEC>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((place_code_kernel<128, VEC>), grid, block, 0, s, a);
}

}  // namespace

extern "C" {

int aura_place_code(const float* z, const float* e, const float* W2t, const float* b2, int64_t N, int64_t P, int64_t D,
                    int64_t k, int32_t* idx, float* act, float* out, float* dense_or_null, void* stream) {
    if (!place_shape_ok(N, P, D, k)) return AURA_E_INVAL;
    if (!z || !e || !W2t || !b2 || !idx || !act || !out) return AURA_E_INVAL;
    if (misaligned(z, 4) || misaligned(e, 4) || misaligned(W2t, 4) || misaligned(b2, 4) || misaligned(idx, 4) ||
        misaligned(act, 4) || misaligned(out, 4) || misaligned(dense_or_null, 4))
        return AURA_E_ALIGN;
    if (N == 0) return AURA_OK;
    PlaceArgs a;
    a.z = z; a.e = e; a.W2t = W2t; a.b2 = b2; a.idx = idx; a.act = act; a.out = out; a.dense = dense_or_null;
    a.N = N; a.P = (int)P; a.D = (int)D; a.k = (int)k;
    const dim3 grid((unsigned)((N + PLACE_WAVES - 1) / PLACE_WAVES));
    const bool vec = D % 4 == 0 && !misaligned(e, 16) && !misaligned(W2t, 16) && !misaligned(b2, 16) &&
                     !misaligned(out, 16);
    if (vec) place_launch<true>(a, grid, static_cast<hipStream_t>(stream));
    else place_launch<false>(a, grid, static_cast<hipStream_t>(stream));
    return aura_check_launch();
}

int aura_place_code_backward(const float* g_out, const float* g_dense_or_null, const int32_t* idx, const float* act,
                             const float* W2t, int64_t N, int64_t P, int64_t D, int64_t k, float* g_z, void* stream) {
    if (!place_shape_ok(N, P, D, k)) return AURA_E_INVAL;
    if (!g_out || !idx || !act || !W2t || !g_z) return AURA_E_INVAL;
    if (misaligned(g_out, 4) || misaligned(g_dense_or_null, 4) || misaligned(idx, 4) || misaligned(act, 4) ||
        misaligned(W2t, 4) || misaligned(g_z, 4))
        return AURA_E_ALIGN;
    if (N == 0) return AURA_OK;
    PlaceBwdArgs a;
    a.g_out = g_out; a.g_dense = g_dense_or_null; a.idx = idx; a.act = act; a.W2t = W2t; a.g_z = g_z;
    a.N = N; a.P = (int)P; a.D = (int)D; a.k = (int)k;
    const dim3 grid((unsigned)((N + PLACE_WAVES - 1) / PLACE_WAVES)), block(64 * PLACE_WAVES);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (D % 4 == 0 && !misaligned(g_out, 16) && !misaligned(W2t, 16))
        hipLaunchKernelGGL((place_code_backward_kernel<true>), grid, block, 0, s, a);
    else
        hipLaunchKernelGGL((place_code_backward_kernel<false>), grid, block, 0, s, a);
    return aura_check_launch();
}

}  // extern "C"
