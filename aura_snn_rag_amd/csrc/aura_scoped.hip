// aura_scoped.hip -- scoped recall: the exact top-k of the reference's combined score over a per-query SUBSET of the
// held rows (a tag, a time window, a strength floor), and the tag stamp of the write paths; gfx950.
// [build-side] no upstream counterpart (the reference drops event_id; metadata column 3 is "reserved").
//
// The rule (include/aura_hip.h states it in full): row r < count is in query i's scope iff its tag (metadata column 3)
// equals the query's tag (or the query takes any tag) and the call's conditions on timestamp and strength hold; the
// result is the top k of the scope by (0.5 cos + 0.3 spatial + 0.2 exp(-(now - ts) / 3600)) * strength, descending,
// equal scores to the lower row, the tail padded with -inf / -1.
//
// A stateless per-call build, then a scan whose work follows the sizes of the scopes:
//   query_norm   1 / max(||q||, 1e-12) per query (one wave each); resets the call's flag
//   count        one pass over meta[0 .. count): per block of 256 rows, how many rows every scope of the call takes
//   scan, base   exclusive prefix of those counts over the blocks of a scope, then over the scopes
//   scatter      the same pass again: row ids to their scope's list, ascending (a row's place is its block's offset
//                plus the number of earlier rows of the block in the same scope: no atomics decide an order)
//   score        grid (query tiles, splits): a tile of up to 64 queries of ONE scope against that scope's list, 128
//                gathered rows at a time on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32, a fixed order along D, so a
//                pair's score bits do not depend on what else is in the call); the combined score in the epilogue; a
//                sorted top-k per query kept in registers across the row tiles (entry j in lane j & 63, slot j >> 6).
//                Split s takes the row tiles s, s + splits, ...: a scope of 100 rows is one tile, whatever the bank holds
//   merge        splits > 1: the splits' lists of a query merged by the same insertion, one wave per query
// Nothing is read back between the launches: the grids follow from host-known sizes and every block sizes its loop
// from the scope's length on the device.  Every row id is range-checked before it becomes an address.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/aura_hip.h"
#include "aura_common.inl"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr int SC_THREADS = 256;
constexpr int SC_BUILD_ROWS = 256;          // rows per block of the scope build (one per thread)
constexpr int SC_MAX_SCOPES = 256;          // distinct scopes per call (the host chunks the queries)
constexpr int SC_MAX_K = 128;               // two list entries per lane
constexpr int SC_MAX_SPLITS = 64;
constexpr int SC_QT = 64;                   // queries per tile
constexpr int SC_RT = 128;                  // gathered rows per tile
constexpr int SC_BK = 64;                   // columns per chunk
constexpr int SC_STRIDE = SC_BK + 4;        // LDS row stride in floats (as aura_diverse.hip)
constexpr int SC_SSTRIDE = SC_RT + 1;       // stride of the score tile [SC_QT][SC_RT]
constexpr int SC_NLD = (SC_QT + SC_RT) * (SC_BK / 4) / SC_THREADS;   // float4 loads per thread and chunk
constexpr int SC_EMPTY = 0x7fffffff;        // row of an unfilled list entry
constexpr int64_t SC_MAX_D = 4096;
constexpr int SC_FLAG_BAD_ROW = 1;          // a scope list held an id outside [0, count)
constexpr int SC_FLAG_BAD_PLAN = 2;         // the plan named a scope, a tile or a query that does not exist

constexpr int sc_lds_bytes() {
    return (((SC_QT + SC_RT) * SC_STRIDE > SC_QT * SC_SSTRIDE) ? (SC_QT + SC_RT) * SC_STRIDE : SC_QT * SC_SSTRIDE) * 4;
}

struct ScLayout {
    int64_t counts, total, base, list, inv_q, part_s, part_r, bytes, blocks, list_cap;
};

inline ScLayout sc_layout(int64_t count, int64_t nq, int64_t k, int64_t n_scopes, int64_t splits) {
    ScLayout w{};
    w.blocks = (count + SC_BUILD_ROWS - 1) / SC_BUILD_ROWS;
    w.list_cap = 2 * count;                 // a row is in at most two scopes of a call: its tag's and "any tag"
    int64_t o = 0;
    w.counts = o; o += aura_align256(n_scopes * w.blocks * 4);
    w.total = o;  o += aura_align256(SC_MAX_SCOPES * 4);
    w.base = o;   o += aura_align256(SC_MAX_SCOPES * 4);
    w.list = o;   o += aura_align256(w.list_cap * 4);
    w.inv_q = o;  o += aura_align256(nq * 4);
    w.part_s = o; o += splits > 1 ? aura_align256(splits * nq * k * 4) : 0;
    w.part_r = o; o += splits > 1 ? aura_align256(splits * nq * k * 4) : 0;
    w.bytes = o;
    return w;
}

struct ScCond {
    int mask;                               // bit 0: ts >= newer, bit 1: ts <= older, bit 2: strength >= min_strength
    float newer, older, min_strength;
};

__device__ __forceinline__ bool sc_pass(const float4 m, const ScCond c) {
    if ((c.mask & 1) && !(m.y >= c.newer)) return false;
    if ((c.mask & 2) && !(m.y <= c.older)) return false;
    if ((c.mask & 4) && !(m.x >= c.min_strength)) return false;
    return true;
}

// The scope code of a row: -2 outside every scope, -1 only in the "any tag" scope (index 0 when the call has one), else
// the index of its tag's scope.  s_tags: the call's scope tags in LDS, ascending, "any" = -1 first.
__device__ __forceinline__ int sc_code(const float* __restrict__ meta, int64_t row, int64_t count, const ScCond c,
                                       const int* s_tags, int S) {
    if (row >= count) return -2;
    const float4 m = *reinterpret_cast<const float4*>(meta + row * 4);
    if (!sc_pass(m, c)) return -2;
    const bool any = S > 0 && s_tags[0] == -1;
    const int tag = aura_row_tag(m.w);          // aura_no_tag = -2 equals no scope tag
    int lo = any ? 1 : 0, hi = S;           // first index whose tag is >= tag
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_tags[mid] < tag) lo = mid + 1; else hi = mid;
    }
    if (lo < S && s_tags[lo] == tag) return lo;
    return any ? -1 : -2;
}

// 1 / ||q||, summed unfused with a 64-stride.  aura_knn.hip's row_inv_norm_kernel uses an fmaf chain over float4s: the two
// differ in the last bits, and merging them would move scoped scores.
__global__ __launch_bounds__(SC_THREADS) void sc_query_norm_kernel(const float* __restrict__ queries, int64_t nq,
                                                                   int64_t D, float* __restrict__ inv_q,
                                                                   int32_t* __restrict__ flag) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (blockIdx.x == 0 && threadIdx.x == 0) *flag = 0;
    const int64_t q = (int64_t)blockIdx.x * 4 + wave;
    if (q >= nq) return;
    float s = 0.0f;
    for (int64_t c = lane; c < D; c += 64) {
        const float v = queries[q * D + c];
        s = s + v * v;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s = s + __shfl_xor(s, off);
    if (lane == 0) inv_q[q] = 1.0f / fmaxf(sqrtf(s), 1e-12f);
}

__global__ __launch_bounds__(SC_THREADS) void sc_count_kernel(const float* __restrict__ meta, int64_t count, ScCond c,
                                                              const int32_t* __restrict__ scope_tags, int S,
                                                              int32_t* __restrict__ counts, int64_t blocks) {
    __shared__ int s_tags[SC_MAX_SCOPES];
    __shared__ int s_hist[SC_MAX_SCOPES];
    const int tid = threadIdx.x;
    s_tags[tid] = tid < S ? scope_tags[tid] : SC_EMPTY;
    s_hist[tid] = 0;
    __syncthreads();
    const int code = sc_code(meta, (int64_t)blockIdx.x * SC_BUILD_ROWS + tid, count, c, s_tags, S);
    if (code != -2) {
        if (s_tags[0] == -1) atomicAdd(&s_hist[0], 1);          // (integer counts: the order of the adds is immaterial)
        if (code >= 0) atomicAdd(&s_hist[code], 1);
    }
    __syncthreads();
    if (tid < S) counts[(int64_t)tid * blocks + blockIdx.x] = s_hist[tid];
}

// block s: counts[s][0 .. blocks) -> their exclusive prefix, total[s] = the sum
__global__ __launch_bounds__(SC_THREADS) void sc_scan_kernel(int32_t* __restrict__ counts, int64_t blocks,
                                                             int32_t* __restrict__ total) {
    __shared__ int s_sum[SC_THREADS];
    const int tid = threadIdx.x;
    int32_t* c = counts + (int64_t)blockIdx.x * blocks;
    const int64_t per = (blocks + SC_THREADS - 1) / SC_THREADS;
    const int64_t lo = tid * per < blocks ? tid * per : blocks;
    const int64_t hi = lo + per < blocks ? lo + per : blocks;
    int sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += c[i];
    s_sum[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < SC_THREADS; ++t) {
            const int v = s_sum[t];
            s_sum[t] = run;
            run += v;
        }
        total[blockIdx.x] = run;
    }
    __syncthreads();
    int run = s_sum[tid];
    for (int64_t i = lo; i < hi; ++i) {
        const int v = c[i];
        c[i] = run;
        run += v;
    }
}

__global__ void sc_base_kernel(const int32_t* __restrict__ total, int S, int32_t* __restrict__ base) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int run = 0;
    for (int s = 0; s < S; ++s) {
        base[s] = run;
        run += total[s];
    }
}

__global__ __launch_bounds__(SC_THREADS) void sc_scatter_kernel(const float* __restrict__ meta, int64_t count, ScCond c,
                                                                const int32_t* __restrict__ scope_tags, int S,
                                                                const int32_t* __restrict__ counts, int64_t blocks,
                                                                const int32_t* __restrict__ base,
                                                                int32_t* __restrict__ list, int64_t list_cap) {
    __shared__ int s_tags[SC_MAX_SCOPES];
    __shared__ int s_code[SC_BUILD_ROWS];
    __shared__ u64 s_bal[SC_THREADS / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    s_tags[tid] = tid < S ? scope_tags[tid] : SC_EMPTY;
    __syncthreads();
    const int64_t row = (int64_t)blockIdx.x * SC_BUILD_ROWS + tid;
    const int code = sc_code(meta, row, count, c, s_tags, S);
    s_code[tid] = code;
    const u64 bal = __ballot(code != -2);
    if (lane == 0) s_bal[wave] = bal;
    __syncthreads();
    if (code == -2) return;
    if (s_tags[0] == -1) {                  // the "any tag" scope takes every row that passes the conditions
        int rank = (int)__popcll(bal & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) rank += (int)__popcll(s_bal[w]);
        const int64_t pos = (int64_t)base[0] + counts[blockIdx.x] + rank;
        if (pos >= 0 && pos < list_cap) list[pos] = (int32_t)row;
    }
    if (code >= 0) {
        int rank = 0;
        for (int t = 0; t < tid; ++t) rank += s_code[t] == code ? 1 : 0;
        const int64_t pos = (int64_t)base[code] + counts[(int64_t)code * blocks + blockIdx.x] + rank;
        if (pos >= 0 && pos < list_cap) list[pos] = (int32_t)row;
    }
}

// ---- the sorted top-k list of one query, spread over a wave: entry j in lane j & 63, slot j >> 6
__device__ __forceinline__ bool sc_better(float av, int ar, float bv, int br) {
    return av > bv || (av == bv && ar < br);
}

__device__ __forceinline__ void sc_insert(float& s0, int& r0, float& s1, int& r1, float cv, int cr, int lane) {
    float p0s = __shfl_up(s0, 1);
    int p0r = __shfl_up(r0, 1);
    float p1s = __shfl_up(s1, 1);
    int p1r = __shfl_up(r1, 1);
    const float es = __shfl(s0, 63);
    const int er = __shfl(r0, 63);
    if (lane == 0) { p1s = es; p1r = er; }
    // an entry that beats the candidate stays; the first that does not takes the candidate; the rest move down by one
    const bool keep0 = sc_better(s0, r0, cv, cr);
    const bool prev0 = lane == 0 ? true : sc_better(p0s, p0r, cv, cr);
    const bool keep1 = sc_better(s1, r1, cv, cr);
    const bool prev1 = sc_better(p1s, p1r, cv, cr);
    s0 = keep0 ? s0 : (prev0 ? cv : p0s);
    r0 = keep0 ? r0 : (prev0 ? cr : p0r);
    s1 = keep1 ? s1 : (prev1 ? cv : p1s);
    r1 = keep1 ? r1 : (prev1 ? cr : p1r);
}

// entry k - 1: what a candidate has to beat
__device__ __forceinline__ void sc_kth(float s0, int r0, float s1, int r1, int k, float& ts, int& tr) {
    const int j = k - 1;
    if (j < 64) { ts = __shfl(s0, j); tr = __shfl(r0, j); }
    else { ts = __shfl(s1, j - 64); tr = __shfl(r1, j - 64); }
}

__device__ __forceinline__ void sc_store_list(float s0, int r0, float s1, int r1, int k, int lane,
                                              float* __restrict__ ds, int32_t* __restrict__ dr) {
    if (lane < k) {
        ds[lane] = r0 == SC_EMPTY ? -INFINITY : s0;
        dr[lane] = r0 == SC_EMPTY ? -1 : r0;
    }
    if (lane + 64 < k) {
        ds[lane + 64] = r1 == SC_EMPTY ? -INFINITY : s1;
        dr[lane + 64] = r1 == SC_EMPTY ? -1 : r1;
    }
}

struct ScArgs {
    const float* bank; const float* inv_norm; const float* meta; const float* loc;
    const float* queries; const float* q_loc; const float* inv_q;
    const int32_t* tile_scope; const int32_t* tile_q0; const int32_t* tile_nq; const int32_t* q_order;
    const int32_t* total; const int32_t* base; const int32_t* list;
    int64_t count, D, nq, list_cap;
    int sdims, S, k, splits;
    float now;
    float* dst_s; int32_t* dst_r;           // [splits][nq][k]
    int32_t* flag;
};

template <bool VEC>
__global__ __launch_bounds__(SC_THREADS) void sc_score_kernel(ScArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];   // [SC_QT + SC_RT][SC_STRIDE], then [SC_QT][SC_SSTRIDE]
    __shared__ int s_row[SC_RT];
    __shared__ int s_q[SC_QT];
    __shared__ float s_iq[SC_QT];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 31, lh = lane >> 5;
    const int tile = blockIdx.x, split = blockIdx.y;

    const int sc = a.tile_scope[tile], q0 = a.tile_q0[tile], nqt = a.tile_nq[tile];
    if (sc < 0 || sc >= a.S || q0 < 0 || nqt < 1 || nqt > SC_QT || (int64_t)q0 + nqt > a.nq) {   // block-uniform
        if (tid == 0) atomicOr(a.flag, SC_FLAG_BAD_PLAN);
        return;
    }
    if (tid < SC_QT) {
        int qi = -1;
        if (tid < nqt) {
            qi = a.q_order[q0 + tid];
            if (qi < 0 || qi >= a.nq) { qi = -1; atomicOr(a.flag, SC_FLAG_BAD_PLAN); }
        }
        s_q[tid] = qi;
        s_iq[tid] = qi >= 0 ? a.inv_q[qi] : 0.0f;
    }
    int64_t n_s = a.total[sc];
    const int64_t lbase = a.base[sc];
    if (n_s < 0 || lbase < 0 || lbase + n_s > a.list_cap) {
        if (tid == 0) atomicOr(a.flag, SC_FLAG_BAD_PLAN);
        n_s = 0;
    }
    const int64_t ntiles = (n_s + SC_RT - 1) / SC_RT;

    // the lists of this wave's 16 queries
    constexpr int QPW = SC_QT / 4;
    float ls0[QPW], ls1[QPW];
    int lr0[QPW], lr1[QPW];
#pragma unroll
    for (int j = 0; j < QPW; ++j) { ls0[j] = ls1[j] = -INFINITY; lr0[j] = lr1[j] = SC_EMPTY; }
    __syncthreads();

    const int64_t KT = (a.D + SC_BK - 1) / SC_BK;
    for (int64_t t = split; t < ntiles; t += a.splits) {
        if (tid < SC_RT) {
            const int64_t i = t * SC_RT + tid;
            int r = -1;
            if (i < n_s) {
                r = a.list[lbase + i];
                if (r < 0 || (int64_t)r >= a.count) {            // the only place a list entry becomes a row
                    atomicOr(a.flag, SC_FLAG_BAD_ROW);
                    r = -1;
                }
            }
            s_row[tid] = r;
        }
        __syncthreads();

        // ---- dot products: 64 queries x 128 rows, wave w owns rows 32 w .. 32 w + 31
        float4 pre[SC_NLD];
        auto gload = [&](int64_t k0) {
#pragma unroll
            for (int i = 0; i < SC_NLD; ++i) {
                const int f = tid + i * SC_THREADS;
                const int rr = f >> 4, c = (f & 15) * 4;
                const int id = rr < SC_QT ? s_q[rr] : s_row[rr - SC_QT];
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (id >= 0 && k0 + c < a.D) {
                    const float* p = (rr < SC_QT ? a.queries : a.bank) + (int64_t)id * a.D + k0 + c;
                    if (VEC) {                                   // D % 4 == 0: the 16 bytes lie inside the row
                        v = *reinterpret_cast<const float4*>(p);
                    } else {
                        const int64_t left = a.D - k0 - c;
                        v.x = p[0];
                        if (left > 1) v.y = p[1];
                        if (left > 2) v.z = p[2];
                        if (left > 3) v.w = p[3];
                    }
                }
                pre[i] = v;
            }
        };
        f32x16 acc0, acc1;
#pragma unroll
        for (int e = 0; e < 16; ++e) { acc0[e] = 0.0f; acc1[e] = 0.0f; }
        gload(0);
        for (int64_t kt = 0; kt < KT; ++kt) {
#pragma unroll
            for (int i = 0; i < SC_NLD; ++i) {
                const int f = tid + i * SC_THREADS;
                *reinterpret_cast<float4*>(smem + (f >> 4) * SC_STRIDE + (f & 15) * 4) = pre[i];
            }
            __syncthreads();
            if (kt + 1 < KT) gload((kt + 1) * SC_BK);
            // lane (li, lh) feeds A[query li][k] and B[k][row li] with the columns 8 kk + 4 lh .. + 3 of a step
            const float* qa = smem + li * SC_STRIDE + 4 * lh;
            const float* qb = smem + (32 + li) * SC_STRIDE + 4 * lh;
            const float* rb = smem + (SC_QT + wave * 32 + li) * SC_STRIDE + 4 * lh;
#pragma unroll
            for (int kk = 0; kk < SC_BK / 8; ++kk) {
                const float4 a0 = *reinterpret_cast<const float4*>(qa + kk * 8);
                const float4 a1 = *reinterpret_cast<const float4*>(qb + kk * 8);
                const float4 b = *reinterpret_cast<const float4*>(rb + kk * 8);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b.x, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b.x, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b.y, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b.y, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, b.z, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, b.z, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, b.w, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, b.w, acc1, 0, 0, 0);
            }
            __syncthreads();
        }

        // ---- epilogue: the combined score (aura_common.inl) into the score tile, which takes the
        // staging buffer's place (barrier above).  Accumulator element e of lane (li, lh): query (e & 3) + 8 (e >> 2)
        // + 4 lh of its half, row li of the wave's 32
        {
            const int lrow = wave * 32 + li;
            const int r = s_row[lrow];
            float inv_m = 0.f, strength = 0.f, tw = 0.f;
            float lx[4] = {0.f, 0.f, 0.f, 0.f};
            if (r >= 0) {
                inv_m = a.inv_norm[r];
                const float4 m = *reinterpret_cast<const float4*>(a.meta + (int64_t)r * 4);
                strength = m.x;
                tw = aura_time_weight(a.now, m.y);
                if (a.q_loc)
                    for (int d = 0; d < a.sdims && d < 4; ++d) lx[d] = a.loc[(int64_t)r * a.sdims + d];
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int ql = h * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                    const int qi = s_q[ql];
                    // aura_score_spatial (aura_common.inl), written out: the call makes this kernel 32 instructions longer
                    const float sim = (h ? acc1[e] : acc0[e]) * s_iq[ql] * inv_m;
                    float comb = 0.5f * sim;
                    if (a.q_loc && qi >= 0) {
                        float d2 = 0.0f;
                        for (int d = 0; d < a.sdims && d < 4; ++d) {
                            const float df = lx[d] - a.q_loc[(int64_t)qi * a.sdims + d];
                            d2 = d2 + df * df;
                        }
                        comb = comb + 0.3f * (1.0f / (1.0f + sqrtf(d2)));
                    }
                    comb = (comb + tw) * strength;
                    smem[ql * SC_SSTRIDE + lrow] = comb;
                }
            }
        }
        __syncthreads();

        // ---- selection: wave w merges the tile into the lists of queries 16 w .. 16 w + 15
#pragma unroll
        for (int j = 0; j < QPW; ++j) {
            const int ql = wave * QPW + j;
            if (s_q[ql] < 0) continue;                           // wave-uniform
            float ts;
            int tr;
            sc_kth(ls0[j], lr0[j], ls1[j], lr1[j], a.k, ts, tr);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int rr = s_row[lane + 64 * h];
                float v = smem[ql * SC_SSTRIDE + lane + 64 * h];
                if (!(v == v)) v = -INFINITY;                    // a NaN score ranks last
                const int r = rr >= 0 ? rr : SC_EMPTY;
                u64 m = __ballot(r != SC_EMPTY && sc_better(v, r, ts, tr));
                while (m) {
                    const int b = __ffsll(m) - 1;
                    const float cv = __shfl(v, b);
                    const int cr = __shfl(r, b);
                    sc_insert(ls0[j], lr0[j], ls1[j], lr1[j], cv, cr, lane);
                    sc_kth(ls0[j], lr0[j], ls1[j], lr1[j], a.k, ts, tr);
                    m &= m - 1;
                    m &= __ballot(sc_better(v, r, ts, tr));
                }
            }
        }
        __syncthreads();                                         // the next tile overwrites s_row and the score tile
    }

    // a split without a tile of its own still leaves its (empty) lists: the merge reads every split
#pragma unroll
    for (int j = 0; j < QPW; ++j) {
        const int qi = s_q[wave * QPW + j];
        if (qi < 0) continue;
        const int64_t o = ((int64_t)split * a.nq + qi) * a.k;
        sc_store_list(ls0[j], lr0[j], ls1[j], lr1[j], a.k, lane, a.dst_s + o, a.dst_r + o);
    }
}

// one wave per query: the splits' sorted lists -> the query's top k
__global__ __launch_bounds__(SC_THREADS) void sc_merge_kernel(const float* __restrict__ part_s,
                                                              const int32_t* __restrict__ part_r, int64_t nq, int k,
                                                              int splits, float* __restrict__ out_s,
                                                              int32_t* __restrict__ out_r) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + wave;
    if (q >= nq) return;
    float s0 = -INFINITY, s1 = -INFINITY, ts = -INFINITY;
    int r0 = SC_EMPTY, r1 = SC_EMPTY, tr = SC_EMPTY;
    for (int p = 0; p < splits; ++p) {
        const int64_t o = ((int64_t)p * nq + q) * k;
        for (int j = 0; j < k; ++j) {                            // (every lane reads the same entry: wave-uniform)
            const float cv = part_s[o + j];
            const int cr = part_r[o + j];
            if (cr < 0 || !sc_better(cv, cr, ts, tr)) break;     // a sorted list: nothing behind it gets in either
            sc_insert(s0, r0, s1, r1, cv, cr, lane);
            sc_kth(s0, r0, s1, r1, k, ts, tr);
        }
    }
    sc_store_list(s0, r0, s1, r1, k, lane, out_s + q * k, out_r + q * k);
}

__global__ void sc_set_tags_kernel(float* __restrict__ meta, int64_t count, const int64_t* __restrict__ slots,
                                   const int32_t* __restrict__ tags, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t s = slots[i];
    const int32_t t = tags[i];
    if (s < 0 || s >= count || t < 0 || t >= (1 << 24)) return;  // checked before it becomes an address
    meta[s * 4 + 3] = (float)t;
}

}  // namespace

extern "C" {

int aura_bank_set_tags(float* meta, int64_t count, const int64_t* slots, const int32_t* tags, int64_t n, void* stream) {
    if (n < 0 || count < 0) return AURA_E_INVAL;
    if (n == 0) return AURA_OK;
    if (!meta || !slots || !tags) return AURA_E_INVAL;
    if (n > 0x7fffffffLL * 256) return AURA_E_INVAL;
    hipLaunchKernelGGL(sc_set_tags_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), meta, count, slots, tags, n);
    return aura_check_launch();
}

int64_t aura_knn_scoped_workspace_bytes(int64_t count, int64_t nq, int64_t k, int64_t n_scopes, int64_t splits) {
    if (count < 1 || count > 0x3fffffffLL || nq < 0 || nq > 0x7fffffffLL || k < 1 || k > SC_MAX_K || n_scopes < 1 ||
        n_scopes > SC_MAX_SCOPES || splits < 1 || splits > SC_MAX_SPLITS)
        return -1;
    return sc_layout(count, nq, k, n_scopes, splits).bytes;
}

int aura_knn_search_scoped(const float* bank, const float* inv_norm, const float* meta, const float* loc,
                           int spatial_dims, const float* queries, const float* q_loc, float now, int64_t count,
                           int64_t D, int64_t nq, int k, const int32_t* plan, int64_t n_scopes, int64_t n_tiles,
                           int64_t splits, int conditions, float newer_than, float older_than, float min_strength,
                           float* out_scores, int32_t* out_rows, void* workspace, int64_t workspace_bytes,
                           int32_t* flag_out, void* stream) {
    const int64_t need = aura_knn_scoped_workspace_bytes(count, nq, k, n_scopes, splits);
    if (need < 0 || workspace_bytes < need || !workspace) return AURA_E_INVAL;
    if (D < 1 || D > SC_MAX_D || n_tiles < 0 || n_tiles > nq || (conditions & ~7)) return AURA_E_INVAL;
    if (newer_than != newer_than || older_than != older_than || min_strength != min_strength) return AURA_E_INVAL;
    if (q_loc && (!loc || spatial_dims <= 0 || spatial_dims > 4)) return AURA_E_INVAL;
    if (!flag_out) return AURA_E_INVAL;
    if (nq == 0) return AURA_OK;
    if (n_tiles < 1 || !bank || !inv_norm || !meta || !queries || !plan || !out_scores || !out_rows) return AURA_E_INVAL;
    if ((reinterpret_cast<uintptr_t>(workspace) & 255) || (reinterpret_cast<uintptr_t>(meta) & 15)) return AURA_E_ALIGN;
    const bool vec = D % 4 == 0 && !(reinterpret_cast<uintptr_t>(bank) & 15) && !(reinterpret_cast<uintptr_t>(queries) & 15);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const ScLayout w = sc_layout(count, nq, k, n_scopes, splits);
    char* ws = static_cast<char*>(workspace);
    int32_t* counts = reinterpret_cast<int32_t*>(ws + w.counts);
    int32_t* total = reinterpret_cast<int32_t*>(ws + w.total);
    int32_t* base = reinterpret_cast<int32_t*>(ws + w.base);
    int32_t* list = reinterpret_cast<int32_t*>(ws + w.list);
    float* inv_q = reinterpret_cast<float*>(ws + w.inv_q);
    const int32_t* scope_tags = plan;
    const int S = (int)n_scopes;
    const ScCond c{conditions, newer_than, older_than, min_strength};
    int rc;

    hipLaunchKernelGGL(sc_query_norm_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(SC_THREADS), 0, s, queries, nq, D,
                       inv_q, flag_out);
    if ((rc = aura_check_launch())) return rc;
    hipLaunchKernelGGL(sc_count_kernel, dim3((unsigned)w.blocks), dim3(SC_THREADS), 0, s, meta, count, c, scope_tags,
                       S, counts, w.blocks);
    if ((rc = aura_check_launch())) return rc;
    hipLaunchKernelGGL(sc_scan_kernel, dim3((unsigned)S), dim3(SC_THREADS), 0, s, counts, w.blocks, total);
    if ((rc = aura_check_launch())) return rc;
    hipLaunchKernelGGL(sc_base_kernel, dim3(1), dim3(64), 0, s, total, S, base);
    if ((rc = aura_check_launch())) return rc;
    hipLaunchKernelGGL(sc_scatter_kernel, dim3((unsigned)w.blocks), dim3(SC_THREADS), 0, s, meta, count, c,
                       scope_tags, S, counts, w.blocks, base, list, w.list_cap);
    if ((rc = aura_check_launch())) return rc;

    ScArgs a{};
    a.bank = bank; a.inv_norm = inv_norm; a.meta = meta; a.loc = loc; a.queries = queries; a.q_loc = q_loc;
    a.inv_q = inv_q;
    a.tile_scope = plan + n_scopes; a.tile_q0 = a.tile_scope + n_tiles; a.tile_nq = a.tile_q0 + n_tiles;
    a.q_order = a.tile_nq + n_tiles;
    a.total = total; a.base = base; a.list = list;
    a.count = count; a.D = D; a.nq = nq; a.list_cap = w.list_cap;
    a.sdims = spatial_dims; a.S = S; a.k = k; a.splits = (int)splits; a.now = now;
    a.dst_s = splits > 1 ? reinterpret_cast<float*>(ws + w.part_s) : out_scores;
    a.dst_r = splits > 1 ? reinterpret_cast<int32_t*>(ws + w.part_r) : out_rows;
    a.flag = flag_out;
    const dim3 grid((unsigned)n_tiles, (unsigned)splits);
    if (vec) hipLaunchKernelGGL(sc_score_kernel<true>, grid, dim3(SC_THREADS), sc_lds_bytes(), s, a);
    else hipLaunchKernelGGL(sc_score_kernel<false>, grid, dim3(SC_THREADS), sc_lds_bytes(), s, a);
    if ((rc = aura_check_launch())) return rc;
    if (splits > 1) {
        hipLaunchKernelGGL(sc_merge_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(SC_THREADS), 0, s, a.dst_s, a.dst_r,
                           nq, k, (int)splits, out_scores, out_rows);
        if ((rc = aura_check_launch())) return rc;
    }
    return AURA_OK;
}

}  // extern "C"
