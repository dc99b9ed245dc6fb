// aura_consolidate.hip -- consolidating writes: which rows of a batch repeat a stored memory or an earlier row
// of the same batch (aura_bank_find_repeats), and the timestamp refresh of the rows that were repeated
// (aura_bank_touch), for gfx950.  [build-side] no upstream counterpart.
//
// The rule (include/aura_hip.h states it in full): cos(x, y) = fp32 dot product of the two rows, each scaled by
// 1 / max(||.||, 1e-12); stored_target[i] = the held row of largest cos(f_i, r) >= tau (equal cosines -> the lowest
// r), else -1; rows without a stored target are walked in order and repeat the KEPT earlier row of largest cosine
// >= tau (equal -> the lowest j), else they are kept; rows with a NaN / Inf component or of norm 0 are kept and are
// nobody's target.  With batch_tags the call applies the same rule within tags: a held row is eligible for a batch
// row only when its tag (metadata column 3) equals the batch row's, an in-batch pair only when both rows carry one tag.
// The predicate is one SCOPED template parameter of the scan, dense and walk kernels: it sits where a pair is decided
// (before a survivor is appended, before the packed atomicMax, before pend[] is set, before a kept row offers its Gram
// entry), and the unscoped instantiations compile to what they were without it.
//
// Launches of one call (all on the caller's stream, no allocation, no host synchronisation):
//   prep      1 / ||f_i||, the degenerate flag, the counters' reset and -- with an image -- the batch's normalised
//             bf16 rows and the query part of the prefilter's error bound (the two-stage recall's arithmetic);
//   scan      with an image: ONE pass over the bf16 image on the bf16 matrix pipe.  A workgroup of 4 waves holds 128
//             image rows as v_mfma_f32_32x32x16_bf16 A-fragments in registers (a wave: 32 rows x D, read from HBM
//             exactly once, straight into the fragment layout) and streams the batch through LDS in tiles of 32
//             rows (double buffered, XOR-swizzled 16-byte chunks: every ds_read_b128 is conflict-free).  A pair
//             survives when cos_bf16 + err >= tau; survivors are appended to per-query lists (returning atomics:
//             rare).  A second launch re-scores them in fp32 from the fp32 bank and takes the arg-max;
//             without an image: a dense fp32 scan on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32, the form of
//             aura_diverse.hip), per-query maximum by a packed 64-bit atomicMax (ordered cosine bits, ~row);
//   gram      the n x n cosines of the batch on the fp32 matrix pipe (same kernel), lower triangle; a row with an
//             eligible pair >= tau is marked pending;
//   walk      one workgroup: rows that are not pending are decided at once, the pending ones (almost always none)
//             are walked in order, one workgroup arg-max each.
// Every matrix instruction is a compiler builtin (hipcc pads the hazards); every row id is range-checked before it
// becomes an address.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/aura_hip.h"
#include "aura_common.inl"

#pragma clang fp contract(off)

namespace {

typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned long long u64;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));     // (HIP's uint4 is a struct: arrays of it stay in scratch)

constexpr int CS_MAX_BATCH = 1024;
constexpr int CS_MAX_IMAGE_D = 768;
constexpr int CS_CAP = 256;              // survivor slots per batch row
constexpr int CS_BK = 64;                // dense scan: columns per chunk
constexpr int CS_STRIDE = CS_BK + 4;     // LDS row stride in floats (as aura_diverse.hip)

inline int pad_batch(int64_t n) { return (int)((n + 127) / 128 * 128); }

struct Workspace {
    u64* best;          // [n_pad] packed (ordered cosine bits, ~row), 0 = none
    int32_t* cnt;       // [n_pad] survivors appended per batch row
    int32_t* pend;      // [n_pad] the row has an eligible in-batch pair >= tau
    int32_t* okf;       // [n_pad] the row is not degenerate
    int32_t* elig;      // [n_pad] not degenerate and without a stored target
    float* qinv;        // [n_pad]
    float* eq;          // [n_pad] query part of the prefilter's error bound (NaN: never survives)
    uint16_t* qhat;     // [n_pad][768] normalised bf16 rows
    int32_t* list;      // [n_pad][CS_CAP]
    float* gram;        // [n_pad][n_pad]
    int32_t* tag;       // [n_pad] scoped calls: the batch rows' tags, -1 for padding and for a tag outside [0, 2^24)
    int64_t bytes;
};

inline Workspace carve(void* base, int n_pad) {
    Workspace w;
    char* p = static_cast<char*>(base);
    int64_t o = 0;
    auto take = [&](int64_t b) { char* r = p ? p + o : nullptr; o += aura_align256(b); return r; };
    w.best = reinterpret_cast<u64*>(take(8LL * n_pad));
    w.cnt = reinterpret_cast<int32_t*>(take(4LL * n_pad));
    w.pend = reinterpret_cast<int32_t*>(take(4LL * n_pad));
    w.okf = reinterpret_cast<int32_t*>(take(4LL * n_pad));
    w.elig = reinterpret_cast<int32_t*>(take(4LL * n_pad));
    w.qinv = reinterpret_cast<float*>(take(4LL * n_pad));
    w.eq = reinterpret_cast<float*>(take(4LL * n_pad));
    w.qhat = reinterpret_cast<uint16_t*>(take(2LL * n_pad * CS_MAX_IMAGE_D));
    w.list = reinterpret_cast<int32_t*>(take(4LL * n_pad * CS_CAP));
    w.gram = reinterpret_cast<float*>(take(4LL * n_pad * n_pad));
    w.tag = reinterpret_cast<int32_t*>(take(4LL * n_pad));
    w.bytes = o;
    return w;
}

// c >= tau > 0: the bits of a positive float ascend with it.  Equal cosines -> the larger ~row = the lower row.
__device__ __forceinline__ u64 cs_pack(float c, int row) {
    return ((u64)(__float_as_uint(c) | 0x80000000u) << 32) | (u64)(uint32_t)(~row);
}
__device__ __forceinline__ float cs_key_cos(u64 key) { return __uint_as_float((uint32_t)(key >> 32) & 0x7fffffffu); }
__device__ __forceinline__ int cs_key_row(u64 key) { return (int)(~(uint32_t)key); }
__device__ __forceinline__ u64 cs_max(u64 a, u64 b) { return a > b ? a : b; }
__device__ __forceinline__ u64 cs_shfl_xor(u64 v, int off) {
    const uint32_t lo = __shfl_xor((uint32_t)v, off), hi = __shfl_xor((uint32_t)(v >> 32), off);
    return ((u64)hi << 32) | lo;
}

// The tag of held row `row`; aura_no_tag = -2 (no batch tag equals it: those are >= -1) for anything that is no tag.
__device__ __forceinline__ int cs_row_tag(const float* __restrict__ meta, int64_t row) {
    return aura_row_tag(meta[row * 4 + 3]);
}

// ---- prep: one wave per batch row (rows [n, n_pad) are padding)
__global__ __launch_bounds__(256) void cs_prep_kernel(const float* __restrict__ x, int n, int n_pad, int64_t D,
                                                      int qstride, Workspace w, int with_image,
                                                      int32_t* __restrict__ overflow,
                                                      const int32_t* __restrict__ batch_tags) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blockIdx.x == 0 && threadIdx.x == 0) *overflow = 0;
    if (q >= n_pad) return;
    float s = 0.0f;
    if (q < n)
        for (int64_t k = lane; k < D; k += 64) { const float u = x[(int64_t)q * D + k]; s = fmaf(u, u, s); }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    const float iq = 1.0f / fmaxf(sqrtf(s), 1e-12f);
    const bool ok = q < n && s > 0.0f && s < INFINITY;        // NaN / Inf, zero rows, fp32 over/underflow of s: kept
    float e2 = 0.0f;
    if (with_image) {
        uint16_t* const dst = w.qhat + (int64_t)q * qstride;
        for (int c = lane; c < qstride / 8; c += 64) {
            f32x8 v;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int64_t k = 8 * (int64_t)c + e;
                v[e] = (ok && k < D) ? x[(int64_t)q * D + k] * iq : 0.0f;
            }
            f32x8 back;
            if (with_image == 2) {            // IEEE half under the image's rule: nearest-even, |x| < 2^-14 stored as 0
                f32x8 vf = v;
#pragma unroll
                for (int e = 0; e < 8; ++e) vf[e] = fabsf(v[e]) < 6.103515625e-05f ? 0.0f : v[e];
                const f16x8 hv = __builtin_convertvector(vf, f16x8);
                *reinterpret_cast<f16x8*>(dst + 8 * c) = hv;
                back = __builtin_convertvector(hv, f32x8);
            } else {
                const bf16x8 bv = __builtin_convertvector(v, bf16x8);
                *reinterpret_cast<bf16x8*>(dst + 8 * c) = bv;
                back = __builtin_convertvector(bv, f32x8);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float d = back[e] - v[e]; e2 = fmaf(d, d, e2); }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) e2 += __shfl_xor(e2, off);
    }
    if (lane == 0) {
        w.qinv[q] = q < n ? iq : 0.0f;
        w.eq[q] = ok ? aura_eq_from_e2(e2, (float)D) : NAN;
        w.okf[q] = ok ? 1 : 0;
        w.elig[q] = 0;
        w.cnt[q] = 0;
        w.pend[q] = 0;
        w.best[q] = 0;
        if (batch_tags) {
            const int32_t t = q < n ? batch_tags[q] : -1;
            w.tag[q] = (t >= 0 && t < (1 << 24)) ? t : -1;
        }
    }
}

// ---- image scan.  KS = 16-column steps held per image row (a multiple of 8: the swizzle works on 16 chunks).
// F16: image and batch rows are IEEE half (the list-sorted image of the inverted lists), rho is that image's rho16 and
// the MFMA the f16 one of the same shape.
template <int KS, bool SCOPED, bool F16>
__global__ __launch_bounds__(256, 1) void cs_scan_kernel(const uint16_t* __restrict__ image,
                                                         const int32_t* __restrict__ image_rows, int64_t n_image,
                                                         int64_t N, int D, const float* __restrict__ rho,
                                                         const uint16_t* __restrict__ qhat,
                                                         const float* __restrict__ eq, int n_tiles, float tau,
                                                         float fix, int32_t* __restrict__ cnt,
                                                         int32_t* __restrict__ list, const float* __restrict__ meta,
                                                         const int32_t* __restrict__ btag) {
    constexpr int CPR = 2 * KS;                 // 16-byte chunks per batch row
    constexpr int TILE = 32 * CPR;              // chunks per tile of 32 batch rows
    constexpr int PF = TILE / 256;              // chunks a thread stages per tile
    extern __shared__ u32x4 cs_smem[];          // [2][32][CPR], chunk index XOR (row & 15)
    __shared__ float s_eq[2][32];               // the tile's query parts of the bound, staged with it
    __shared__ int s_tag[2][32];                // SCOPED: the tile's batch tags (unused and dropped otherwise)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r = lane & 31, h = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * 128 + wave * 32;

    // the wave's 32 image rows as A-fragments: lane (r, h) holds row r, columns 16 kk + 8 h .. + 7
    bf16x8 a[KS];
    {
        const int64_t irow = row0 + r;
        const bool rv = irow < n_image;
        const u32x4* src = reinterpret_cast<const u32x4*>(image + (rv ? irow : 0) * D);
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
            u32x4 v = {0u, 0u, 0u, 0u};
            if (rv && 16 * kk + 8 * h < D) v = src[2 * kk + h];           // D % 8 == 0: inside the row
            a[kk] = __builtin_bit_cast(bf16x8, v);
        }
    }
    // accumulator element e of lane (r, h) is image row (e & 3) + 8 (e >> 2) + 4 h of the wave, batch row r
    float rho_e[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int64_t ir = row0 + (e & 3) + 8 * (e >> 2) + 4 * h;
        float v = NAN;                                                    // NaN: the pair never survives
        if (ir < n_image) {
            const int64_t br = image_rows ? (int64_t)image_rows[ir] : ir;
            if (br >= 0 && br < N) v = rho[br];
        }
        rho_e[e] = v;
    }

    const u32x4* qsrc = reinterpret_cast<const u32x4*>(qhat);
    u32x4 pre[PF];
    float pre_eq = 0.0f;
    int pre_tag = -1;
    auto gload = [&](int t) {
#pragma unroll
        for (int i = 0; i < PF; ++i) pre[i] = qsrc[(int64_t)t * TILE + tid + i * 256];
        if (tid < 32) pre_eq = eq[t * 32 + tid];
        if (SCOPED && tid < 32) pre_tag = btag[t * 32 + tid];
    };
    auto sstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            const int c = tid + i * 256, q = c / CPR, ch = c % CPR;
            cs_smem[buf * TILE + q * CPR + (ch ^ (q & 15))] = pre[i];
        }
        if (tid < 32) s_eq[buf][tid] = pre_eq;
        if (SCOPED && tid < 32) s_tag[buf][tid] = pre_tag;
    };
    gload(0);
    sstore(0);
    __syncthreads();
    const int sw = r & 15;
    for (int t = 0; t < n_tiles; ++t) {
        if (t + 1 < n_tiles) gload(t + 1);
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
        const u32x4* b = cs_smem + (t & 1) * TILE + r * CPR;
        // B-fragments are read four steps ahead of the MFMAs that use them (two register sets of four)
        u32x4 bq[2][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bq[0][j] = b[(2 * j + h) ^ sw];
#pragma unroll
        for (int g = 0; g < KS / 4; ++g) {
            if (g + 1 < KS / 4) {
#pragma unroll
                for (int j = 0; j < 4; ++j) bq[(g + 1) & 1][j] = b[(2 * (4 * (g + 1) + j) + h) ^ sw];
            }
            __builtin_amdgcn_sched_barrier(0);          // (the scheduler sinks the reads to their MFMAs otherwise)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if constexpr (F16)
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a[4 * g + j]),
                                                                 __builtin_bit_cast(f16x8, bq[g & 1][j]), acc, 0, 0, 0);
                else
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[4 * g + j], __builtin_bit_cast(bf16x8, bq[g & 1][j]), acc,
                                                                  0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        // survive: cos_bf16 + rho_r + eq + rho_r eq + fix >= tau
        const int q = t * 32 + r;
        const float eqv = s_eq[t & 1][r];
        const float aq = 1.0f + eqv, tq = tau - eqv - fix;
        if constexpr (SCOPED) {
            // The survivors of the lane as a bit mask, then a loop over the set bits: almost always none.  The tag of
            // the bank row (of image_rows[ir] with a list-sorted image) is read from meta here, in the rare branch,
            // after the range check of br and before the append -- no tag is held across the tile loop, and a pair of
            // another tag never enters a list: other scopes' copies cannot fill the 256 entries.
            uint32_t m = 0;
#pragma unroll
            for (int e = 0; e < 16; ++e) m |= (acc[e] + rho_e[e] * aq >= tq) ? (1u << e) : 0u;
            const int qtag = s_tag[t & 1][r];
            while (m) {
                const int e = __ffs(m) - 1;
                m &= m - 1;
                const int64_t ir = row0 + (e & 3) + 8 * (e >> 2) + 4 * h;
                const int64_t br = image_rows ? (int64_t)image_rows[ir] : ir;
                if (br >= 0 && br < N && cs_row_tag(meta, br) == qtag) {
                    const int pos = atomicAdd(&cnt[q], 1);
                    if (pos < CS_CAP) list[(int64_t)q * CS_CAP + pos] = (int32_t)br;
                }
            }
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                if (acc[e] + rho_e[e] * aq >= tq) {
                    const int64_t ir = row0 + (e & 3) + 8 * (e >> 2) + 4 * h;
                    const int64_t br = image_rows ? (int64_t)image_rows[ir] : ir;      // (valid: rho_e is not NaN)
                    const int pos = atomicAdd(&cnt[q], 1);
                    if (pos < CS_CAP) list[(int64_t)q * CS_CAP + pos] = (int32_t)br;
                }
            }
        }
        if (t + 1 < n_tiles) sstore((t + 1) & 1);
        __syncthreads();
    }
}

// fp32 cosine of batch row q and bank row `row`, one wave: lanes stride the columns, fixed reduction order
__device__ __forceinline__ float cs_wave_cos(const float* __restrict__ f, float iq, const float* __restrict__ b,
                                             float inv, int64_t D, int lane) {
    float s = 0.0f;
    for (int64_t k = lane; k < D; k += 64) s = fmaf(f[k] * iq, b[k] * inv, s);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    return s;
}

__device__ __forceinline__ void cs_finalise(u64 key, int q, const Workspace& w, int32_t* stored_target,
                                            float* cos_out) {
    stored_target[q] = key ? cs_key_row(key) : -1;
    cos_out[q] = key ? cs_key_cos(key) : -INFINITY;
    w.elig[q] = (w.okf[q] && !key) ? 1 : 0;
}

// ---- re-score the survivors of batch row q = blockIdx.x in fp32, arg-max, apply tau
__global__ __launch_bounds__(256) void cs_rescore_kernel(const float* __restrict__ bank,
                                                         const float* __restrict__ inv_norm, int64_t N, int64_t D,
                                                         const float* __restrict__ feats, float tau, Workspace w,
                                                         int32_t* __restrict__ stored_target,
                                                         float* __restrict__ cos_out, int32_t* __restrict__ overflow) {
    __shared__ u64 s_key[4];
    const int q = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = w.cnt[q];
    if (threadIdx.x == 0 && c > CS_CAP) *overflow = 1;         // (every writer stores the same value)
    const int m = c < CS_CAP ? c : CS_CAP;
    const float iq = w.qinv[q];
    u64 key = 0;
    for (int s = wave; s < m; s += 4) {
        const int row = w.list[(int64_t)q * CS_CAP + s];
        if (row < 0 || (int64_t)row >= N) continue;            // the only place a survivor becomes an address
        const float v = cs_wave_cos(feats + (int64_t)q * D, iq, bank + (int64_t)row * D, inv_norm[row], D, lane);
        if (v >= tau) key = cs_max(key, cs_pack(v, row));
    }
    if (lane == 0) s_key[wave] = key;
    __syncthreads();
    if (threadIdx.x == 0)
        cs_finalise(cs_max(cs_max(s_key[0], s_key[1]), cs_max(s_key[2], s_key[3])), q, w, stored_target, cos_out);
}

__global__ __launch_bounds__(256) void cs_finalise_kernel(int n, Workspace w, int32_t* __restrict__ stored_target,
                                                          float* __restrict__ cos_out) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q < n) cs_finalise(w.best[q], q, w, stored_target, cos_out);
}

// ---- dense fp32 cosines of A rows (32 per workgroup) x B rows (128 per workgroup, 32 per wave).
// MODE 0: A = the bank, B = the batch: per-batch-row maximum >= tau into best[] (packed atomicMax).
// MODE 1: A = B = the batch: the lower triangle of the Gram into G, pend[i] = 1 for an eligible pair >= tau.
template <bool VEC>
__device__ __forceinline__ float4 cs_load4(const float* row, int64_t k0, int64_t D, float scale) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!row || k0 >= D) return v;
    if (VEC) {
        v = *reinterpret_cast<const float4*>(row + k0);                 // D % 4 == 0: inside the row
    } else {
        v.x = row[k0];
        if (k0 + 1 < D) v.y = row[k0 + 1];
        if (k0 + 2 < D) v.z = row[k0 + 2];
        if (k0 + 3 < D) v.w = row[k0 + 3];
    }
    v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
    return v;
}

template <bool VEC, int MODE, bool SCOPED>
__global__ __launch_bounds__(256) void cs_dense_kernel(const float* __restrict__ A, const float* __restrict__ ainv,
                                                       int64_t NA, const float* __restrict__ B,
                                                       const float* __restrict__ binv, int nB, int64_t D, float tau,
                                                       u64* __restrict__ best, float* __restrict__ G, int ldg,
                                                       const int32_t* __restrict__ elig, int32_t* __restrict__ pend,
                                                       const float* __restrict__ meta,
                                                       const int32_t* __restrict__ btag) {
    __shared__ __attribute__((aligned(16))) float As[32 * CS_STRIDE];
    __shared__ __attribute__((aligned(16))) float Bs[128 * CS_STRIDE];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 31, lh = lane >> 5;
    const int64_t a0 = (int64_t)blockIdx.x * 32;
    const int b0 = blockIdx.y * 128;
    if (MODE == 1 && (int64_t)b0 > a0 + 31) return;              // above the diagonal: nobody reads it

    const float* asrc[2]; float ascale[2];
    const float* bsrc[8]; float bscale[8];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t row = a0 + ((tid + i * 256) >> 4);
        asrc[i] = row < NA ? A + row * D : nullptr;
        ascale[i] = row < NA ? ainv[row] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int row = b0 + ((tid + i * 256) >> 4);
        bsrc[i] = row < nB ? B + (int64_t)row * D : nullptr;
        bscale[i] = row < nB ? binv[row] : 0.0f;
    }
    float4 apre[2], bpre[8];
    auto gload = [&](int64_t k0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) apre[i] = cs_load4<VEC>(asrc[i], k0 + (tid & 15) * 4, D, ascale[i]);
#pragma unroll
        for (int i = 0; i < 8; ++i) bpre[i] = cs_load4<VEC>(bsrc[i], k0 + (tid & 15) * 4, D, bscale[i]);
    };
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
    const int64_t KT = (D + CS_BK - 1) / CS_BK;
    gload(0);
    for (int64_t kt = 0; kt < KT; ++kt) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
            *reinterpret_cast<float4*>(As + ((tid + i * 256) >> 4) * CS_STRIDE + (tid & 15) * 4) = apre[i];
#pragma unroll
        for (int i = 0; i < 8; ++i)
            *reinterpret_cast<float4*>(Bs + ((tid + i * 256) >> 4) * CS_STRIDE + (tid & 15) * 4) = bpre[i];
        __syncthreads();
        if (kt + 1 < KT) gload((kt + 1) * CS_BK);
        const float* ar = As + li * CS_STRIDE + 4 * lh;
        const float* br = Bs + (wave * 32 + li) * CS_STRIDE + 4 * lh;
#pragma unroll
        for (int kk = 0; kk < CS_BK / 8; ++kk) {
            const float4 av = *reinterpret_cast<const float4*>(ar + kk * 8);
            const float4 bv = *reinterpret_cast<const float4*>(br + kk * 8);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    // element e of lane (li, lh): A row (e & 3) + 8 (e >> 2) + 4 lh, B row li of the wave
    const int j = b0 + wave * 32 + li;
    const int tj = SCOPED ? btag[j] : 0;                              // (j < n_pad: the grid covers exactly n_pad)
    if (MODE == 0) {
        u64 key = 0;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int64_t row = a0 + (e & 3) + 8 * (e >> 2) + 4 * lh;
            if (row < NA && acc[e] >= tau && (!SCOPED || cs_row_tag(meta, row) == tj))
                key = cs_max(key, cs_pack(acc[e], (int)row));
        }
        key = cs_max(key, cs_shfl_xor(key, 32));
        if (lh == 0 && key && j < nB) atomicMax(&best[j], key);
    } else {
        const bool ej = j < nB && elig[j];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int i = (int)a0 + (e & 3) + 8 * (e >> 2) + 4 * lh;       // (i, j < ldg: the grid covers n_pad)
            G[(int64_t)i * ldg + j] = acc[e];
            if (ej && j < i && i < nB && acc[e] >= tau && elig[i] && (!SCOPED || (tj >= 0 && btag[i] == tj)))
                pend[i] = 1;
        }
    }
}

// ---- the ordered walk, one workgroup of 1024 threads: thread i owns batch row i
template <bool SCOPED>
__global__ __launch_bounds__(1024) void cs_walk_kernel(int n, int ldg, float tau, Workspace w,
                                                       int32_t* __restrict__ batch_leader,
                                                       float* __restrict__ cos_out) {
    __shared__ int s_kept[CS_MAX_BATCH];
    __shared__ int s_plist[CS_MAX_BATCH];
    __shared__ int s_wcount[16];
    __shared__ u64 s_key[16];
    __shared__ int s_tag[CS_MAX_BATCH];            // SCOPED: the batch tags (unused and dropped otherwise)
    const int i = threadIdx.x, wave = i >> 6, lane = i & 63;
    if (SCOPED) s_tag[i] = i < n ? w.tag[i] : -1;
    const bool el = i < n && w.elig[i];
    const bool pd = el && w.pend[i];
    s_kept[i] = (el && !pd) ? 1 : 0;
    if (i < n) batch_leader[i] = -1;               // (cos_out: -inf or the stored cosine, written by the scan's finalise)
    const u64 mask = __ballot(pd);
    if (lane == 0) s_wcount[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int v = 0; v < 16; ++v) { const int c = s_wcount[v]; if (v < wave) before += c; total += c; }
    if (pd) s_plist[before + __popcll(mask & ((1ull << lane) - 1ull))] = i;
    __syncthreads();
    for (int p = 0; p < total; ++p) {
        const int row = s_plist[p];
        u64 key = 0;
        if (i < row && s_kept[i] && (!SCOPED || (s_tag[i] >= 0 && s_tag[i] == s_tag[row]))) {
            const float c = w.gram[(int64_t)row * ldg + i];
            if (c >= tau) key = cs_pack(c, i);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) key = cs_max(key, cs_shfl_xor(key, off));
        if (lane == 0) s_key[wave] = key;
        __syncthreads();
        if (i == 0) {
            u64 b = 0;
#pragma unroll
            for (int v = 0; v < 16; ++v) b = cs_max(b, s_key[v]);
            if (b) {
                batch_leader[row] = cs_key_row(b);
                cos_out[row] = cs_key_cos(b);
            } else {
                s_kept[row] = 1;
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void cs_touch_kernel(float* __restrict__ meta, int64_t count,
                                                       const int32_t* __restrict__ rows, int64_t n, float now) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int r = rows[i];
    if (r >= 0 && (int64_t)r < count) meta[(int64_t)r * 4 + 1] = now;      // duplicates store the same value
}

template <int KS, bool SCOPED, bool F16>
int launch_scan(const uint16_t* image, const int32_t* image_rows, int64_t n_image, int64_t N, int D, const float* rho,
                const Workspace& w, int n_tiles, float tau, float fix, const float* meta, hipStream_t s) {
    constexpr int lds = 2 * 32 * 2 * KS * 16;
    if (lds > 64 * 1024) {
        const int rc = aura_ensure_lds_attr(reinterpret_cast<const void*>(&cs_scan_kernel<KS, SCOPED, F16>), lds);
        if (rc != AURA_OK) return rc;
    }
    const unsigned blocks = (unsigned)((n_image + 127) / 128);
    hipLaunchKernelGGL((cs_scan_kernel<KS, SCOPED, F16>), dim3(blocks), dim3(256), lds, s, image, image_rows, n_image, N, D,
                       rho, w.qhat, w.eq, n_tiles, tau, fix, w.cnt, w.list, meta, w.tag);
    return aura_check_launch();
}

template <int MODE, bool SCOPED>
int launch_dense(bool vec, const float* A, const float* ainv, int64_t NA, const float* B, const float* binv, int nB,
                 int n_pad, int64_t D, float tau, const Workspace& w, const float* meta, hipStream_t s) {
    const int64_t rowsA = MODE == 0 ? NA : n_pad;
    const dim3 grid((unsigned)((rowsA + 31) / 32), (unsigned)(n_pad / 128));
    if (vec)
        hipLaunchKernelGGL((cs_dense_kernel<true, MODE, SCOPED>), grid, dim3(256), 0, s, A, ainv, NA, B, binv, nB, D, tau,
                           w.best, w.gram, n_pad, w.elig, w.pend, meta, w.tag);
    else
        hipLaunchKernelGGL((cs_dense_kernel<false, MODE, SCOPED>), grid, dim3(256), 0, s, A, ainv, NA, B, binv, nB, D, tau,
                           w.best, w.gram, n_pad, w.elig, w.pend, meta, w.tag);
    return aura_check_launch();
}


template <bool SCOPED, bool F16 = false>      // F16: the image is IEEE half and `rho` its rho16
int find_repeats_impl(const float* bank, const float* inv_norm, int64_t N, int64_t D, const uint16_t* image_bf16,
                      const int32_t* image_rows, int64_t n_image, const float* rho, const float* feats, int64_t n,
                      float tau, int32_t* stored_target, int32_t* batch_leader, float* cos_out, int32_t* overflow_out,
                      void* workspace, int64_t workspace_bytes, void* stream, const float* meta,
                      const int32_t* batch_tags) {
    const int64_t need = (n < 0 || n > CS_MAX_BATCH) ? -1 : carve(nullptr, pad_batch(n > 0 ? n : 1)).bytes;
    if (need < 0 || N < 0 || N > 0x7fffffffLL || D < 1 || D > 4096) return AURA_E_INVAL;
    if (!(tau > 0.0f && tau <= 1.0f)) return AURA_E_INVAL;
    if (!overflow_out) return AURA_E_INVAL;
    if (n == 0) return AURA_OK;
    if (!feats || !stored_target || !batch_leader || !cos_out || !workspace || workspace_bytes < need) return AURA_E_INVAL;
    if (N > 0 && (!bank || !inv_norm)) return AURA_E_INVAL;
    if (SCOPED && (!batch_tags || (N > 0 && !meta))) return AURA_E_INVAL;
    if (SCOPED && ((reinterpret_cast<uintptr_t>(meta) | reinterpret_cast<uintptr_t>(batch_tags)) & 3)) return AURA_E_ALIGN;
    if (reinterpret_cast<uintptr_t>(workspace) & 255) return AURA_E_ALIGN;
    const bool with_image = image_bf16 != nullptr && N > 0;
    if (with_image) {
        if (D % 8 != 0 || D > CS_MAX_IMAGE_D || n_image < 0 || n_image > 0x7fffffffLL || !rho) return AURA_E_INVAL;
        if (reinterpret_cast<uintptr_t>(image_bf16) & 15) return AURA_E_ALIGN;
    }
    const bool vec = D % 4 == 0 && !(reinterpret_cast<uintptr_t>(bank) & 15) && !(reinterpret_cast<uintptr_t>(feats) & 15);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nn = (int)n, n_pad = pad_batch(n);
    const Workspace w = carve(workspace, n_pad);
    const int ks = with_image ? (int)((D + 127) / 128) * 8 : 0;          // 16-column steps, a multiple of 8
    hipLaunchKernelGGL(cs_prep_kernel, dim3((unsigned)(n_pad / 4)), dim3(256), 0, s, feats, nn, n_pad, D, ks * 16, w,
                       with_image ? (F16 ? 2 : 1) : 0, overflow_out, SCOPED ? batch_tags : nullptr);
    int rc = aura_check_launch();
    if (rc != AURA_OK) return rc;
    if (with_image && n_image > 0) {
        // the error bound's fixed part, as the header states it for the prefilter
        const float fix = 2.0f * (float)D * 5.9604645e-8f + 1e-5f;
        const int n_tiles = (nn + 31) / 32;
        switch (ks) {
        case 8: rc = launch_scan<8, SCOPED, F16>(image_bf16, image_rows, n_image, N, (int)D, rho, w, n_tiles, tau, fix, meta, s); break;
        case 16: rc = launch_scan<16, SCOPED, F16>(image_bf16, image_rows, n_image, N, (int)D, rho, w, n_tiles, tau, fix, meta, s); break;
        case 24: rc = launch_scan<24, SCOPED, F16>(image_bf16, image_rows, n_image, N, (int)D, rho, w, n_tiles, tau, fix, meta, s); break;
        case 32: rc = launch_scan<32, SCOPED, F16>(image_bf16, image_rows, n_image, N, (int)D, rho, w, n_tiles, tau, fix, meta, s); break;
        case 40: rc = launch_scan<40, SCOPED, F16>(image_bf16, image_rows, n_image, N, (int)D, rho, w, n_tiles, tau, fix, meta, s); break;
        default: rc = launch_scan<48, SCOPED, F16>(image_bf16, image_rows, n_image, N, (int)D, rho, w, n_tiles, tau, fix, meta, s); break;
        }
        if (rc != AURA_OK) return rc;
    }
    if (with_image) {
        hipLaunchKernelGGL(cs_rescore_kernel, dim3((unsigned)nn), dim3(256), 0, s, bank, inv_norm, N, D, feats, tau, w,
                           stored_target, cos_out, overflow_out);
    } else {
        if (N > 0) {
            rc = launch_dense<0, SCOPED>(vec, bank, inv_norm, N, feats, w.qinv, nn, n_pad, D, tau, w, meta, s);
            if (rc != AURA_OK) return rc;
        }
        hipLaunchKernelGGL(cs_finalise_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, s, nn, w, stored_target,
                           cos_out);
    }
    rc = aura_check_launch();
    if (rc != AURA_OK) return rc;
    const bool vecq = D % 4 == 0 && !(reinterpret_cast<uintptr_t>(feats) & 15);
    rc = launch_dense<1, SCOPED>(vecq, feats, w.qinv, nn, feats, w.qinv, nn, n_pad, D, tau, w, meta, s);
    if (rc != AURA_OK) return rc;
    hipLaunchKernelGGL(cs_walk_kernel<SCOPED>, dim3(1), dim3(1024), 0, s, nn, n_pad, tau, w, batch_leader, cos_out);
    return aura_check_launch();
}

}  // namespace

extern "C" {

int64_t aura_bank_find_repeats_workspace_bytes(int64_t n) {
    if (n < 0 || n > CS_MAX_BATCH) return -1;
    return carve(nullptr, pad_batch(n > 0 ? n : 1)).bytes;
}

// batch_tags selects the scoped search (meta is ignored without it), image_format the image's format and its rho
int aura_bank_find_repeats(const float* bank, const float* inv_norm, int64_t N, int64_t D, const uint16_t* image,
                           const int32_t* image_rows, int64_t n_image, const float* rho, const float* feats, int64_t n,
                           float tau, int32_t* stored_target, int32_t* batch_leader, float* cos_out,
                           int32_t* overflow_out, void* workspace, int64_t workspace_bytes, const float* meta,
                           const int32_t* batch_tags, int image_format, void* stream) {
    if (image_format != AURA_IMAGE_BF16 && image_format != AURA_IMAGE_F16) return AURA_E_INVAL;
    auto call = [&](auto scoped, auto f16) {
        return find_repeats_impl<decltype(scoped)::value, decltype(f16)::value>(
            bank, inv_norm, N, D, image, image_rows, n_image, rho, feats, n, tau, stored_target, batch_leader, cos_out,
            overflow_out, workspace, workspace_bytes, stream, decltype(scoped)::value ? meta : nullptr, batch_tags);
    };
    using T = std::true_type; using F = std::false_type;
    if (image_format == AURA_IMAGE_BF16) return !batch_tags ? call(F{}, F{}) : call(T{}, F{});
    return !batch_tags ? call(F{}, T{}) : call(T{}, T{});
}

int aura_bank_touch(float* meta, int64_t count, const int32_t* rows, int64_t n, float now, void* stream) {
    if (count < 0 || n < 0 || n > 0x7fffffffLL * 256) return AURA_E_INVAL;
    if (n == 0 || count == 0) return AURA_OK;
    if (!meta || !rows) return AURA_E_INVAL;
    hipLaunchKernelGGL(cs_touch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       meta, count, rows, n, now);
    return aura_check_launch();
}

}  // extern "C"
