// aura_replay.hip -- replay: a seeded, weighted draw of held memories without replacement (gfx950).
// The rule is stated once, in include/aura_hip.h ("Replay"); the comments here are about how it is computed.
//   key pass   one sweep over the 16-byte metadata rows (one float4 per row, four in flight per lane): the scope
//              predicate, Philox4x32-10 on (row, draw) under the seed, three logf, and per row either the draw key d
//              itself (aura_bank_replay_keys) or its REVERSED ordered 32-bit key, ineligible rows at 0xffffffff, with the
//              histogram of its top 12 bits, min / max and the number of eligible rows (aura_bank_replay: pass 0 of
//              the radix selection of aura_select.inl)
//   selection  the n smallest composites  reversed key << 32 | row  (cursor 0) = the n largest d, equal d -> the lower
//              row: the digit passes and the compaction of aura_select.inl, the same code as aura_bank_select_weakest
// The compaction leaves ineligible rows out whatever the threshold says, so a scope of n' < n eligible rows writes n'
// entries; the key pass has filled the n outputs with the padding before.  The tag set (at most 64 sorted tags) travels
// in the kernel arguments and is searched from LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/aura_hip.h"
#include "aura_common.inl"

namespace {
#include "aura_retention.inl"
#include "aura_select.inl"

struct ReplayScope {
    int32_t n_tags;                     // 0: any tag
    int32_t conditions;                 // bit 0 newer_than, 1 older_than, 2 min_strength (aura_knn_search_scoped's)
    float newer_than, older_than, min_strength;
    int32_t tags[AURA_REPLAY_MAX_TAGS]; // strictly ascending
};

struct ReplayDraw {
    uint32_t seed_lo, seed_hi, draw_lo, draw_hi;
    int32_t priority;
    float alpha, now;
};

constexpr uint32_t REPLAY_INELIGIBLE = 0xffffffffu;     // above every reversed ordered key of a finite d

// word 0 of Philox4x32-10, counter (c0, c1, c2, c3), key (k0, k1)
__device__ __forceinline__ uint32_t replay_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                  uint32_t k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1;
        c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}

__device__ __forceinline__ bool replay_in_scope(const float4 m, const ReplayScope& sc, const int32_t* s_tags) {
    bool in = true;
    if (sc.n_tags > 0) {                // binary search of the row's tag (aura_no_tag is below every tag of the set)
        const int t = aura_row_tag(m.w);
        int lo = 0, hi = sc.n_tags;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_tags[mid] < t) lo = mid + 1; else hi = mid;
        }
        in = lo < sc.n_tags && s_tags[lo] == t;
    }
    if (sc.conditions & 1) in = in && m.y >= sc.newer_than;
    if (sc.conditions & 2) in = in && m.y <= sc.older_than;
    if (sc.conditions & 4) in = in && m.x >= sc.min_strength;
    return in;
}

// the rule's steps 1-5 for row r: x >> 9 in *u23, the draw key in *d; returns whether the row is eligible
__device__ __forceinline__ bool replay_row(const float4 m, int64_t r, const ReplayDraw& dr, const ReplayScope& sc,
                                           const int32_t* s_tags, uint32_t* u23, float* d) {
    const uint32_t x = replay_philox((uint32_t)r, (uint32_t)((uint64_t)r >> 32), dr.draw_lo, dr.draw_hi, dr.seed_lo,
                                     dr.seed_hi);
    *u23 = x >> 9;
    const float u = ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-7f;          // 2^-23: exact
    float lw = 0.0f;
    if (dr.priority != AURA_REPLAY_UNIFORM) {
        lw = logf(m.x);
        if (dr.priority == AURA_REPLAY_KEY) lw = lw + -(dr.now - m.y) / 3600.0f;    // aura_recency's argument
    }
    const bool finite = fabsf(lw) < __builtin_inff();                           // (false for NaN)
    float key = dr.alpha * lw - logf(-logf(u));
    if (key == 0.0f) key = 0.0f;                                                // -0 is written as +0
    *d = key;
    return finite && replay_in_scope(m, sc, s_tags);
}

__device__ __forceinline__ float replay_key_of(uint32_t rev) {        // inverse of ~retention_ordered(d), d not NaN
    const uint32_t o = ~rev;
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// SELECT = false: out_d[r] = d (-inf: ineligible), out_u[r] = x >> 9 if asked for.
// SELECT = true: pass 0 of the selection (reversed ordered keys, histogram, min / max), the eligible count and the
// padding of the n outputs.
template <bool SELECT>
__global__ __launch_bounds__(256) void replay_keys_kernel(const float4* __restrict__ meta, int64_t count,
                                                          const ReplayDraw dr, const ReplayScope sc,
                                                          float* __restrict__ out_d, uint32_t* __restrict__ out_u,
                                                          uint32_t* __restrict__ okeys, uint32_t* __restrict__ hist,
                                                          SelState* __restrict__ st0, int64_t n,
                                                          int32_t* __restrict__ out_rows, int64_t* __restrict__ out_comp,
                                                          unsigned long long* __restrict__ out_eligible) {
    __shared__ int32_t s_tags[AURA_REPLAY_MAX_TAGS];
    __shared__ uint32_t s_hist[SELECT ? SEL_BINS : 1];
    __shared__ uint32_t s_mm[2];
    if (threadIdx.x < AURA_REPLAY_MAX_TAGS) s_tags[threadIdx.x] = sc.tags[threadIdx.x];
    if constexpr (SELECT) {
        for (int b = threadIdx.x; b < SEL_BINS; b += 256) s_hist[b] = 0;
        if (threadIdx.x < 2) s_mm[threadIdx.x] = 0;
    }
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * 256;
    if constexpr (SELECT) {
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
            out_rows[i] = -1;
            out_d[i] = -__builtin_inff();
            out_comp[i] = 0x7fffffffffffffffLL;
        }
    }
    uint32_t kmax = 0, kmin_inv = 0, eligible = 0;
    for (int64_t r0 = (int64_t)blockIdx.x * 256 + threadIdx.x; r0 < count; r0 += 4 * stride) {
        float4 m[4];                                        // four 16-byte loads in flight per lane
#pragma unroll
        for (int j = 0; j < 4; ++j)
            m[j] = r0 + j * stride < count ? meta[r0 + j * stride] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t r = r0 + j * stride;
            if (r >= count) break;
            uint32_t u23;
            float d;
            const bool ok = replay_row(m[j], r, dr, sc, s_tags, &u23, &d);
            if constexpr (SELECT) {
                const uint32_t rev = ok ? ~retention_ordered(d) : REPLAY_INELIGIBLE;
                okeys[r] = rev;
                eligible += ok ? 1u : 0u;
                kmax = max(kmax, rev); kmin_inv = max(kmin_inv, ~rev);
                sel_hist_add(s_hist, rev >> 20);
            } else {
                out_d[r] = ok ? d : -__builtin_inff();
                if (out_u) out_u[r] = u23;
            }
        }
    }
    if constexpr (SELECT) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) eligible += (uint32_t)__shfl_xor((int)eligible, off);
        if ((threadIdx.x & 63) == 0 && eligible) atomicAdd(out_eligible, (unsigned long long)eligible);
        sel_minmax_flush(kmax, kmin_inv, s_hist, s_mm, hist, st0);
    }
}

// what the compaction of the draw writes per row: the row, its draw key (back from the reversed ordered key: the bits
// the key pass computed) and the composite; ineligible rows take no part
struct ReplayOut {
    const uint32_t* __restrict__ okeys;
    int32_t* __restrict__ out_rows;
    float* __restrict__ out_d;
    int64_t* __restrict__ out_comp;
    __device__ __forceinline__ bool skip(uint32_t ok, int64_t) const { return ok == REPLAY_INELIGIBLE; }
    __device__ __forceinline__ void write(uint32_t pos, int64_t r) const {
        const uint32_t rev = okeys[r];
        out_rows[pos] = (int32_t)r;
        out_d[pos] = replay_key_of(rev);
        out_comp[pos] = (int64_t)(retention_comp(rev, r, 0, 0) ^ 0x8000000000000000ull);    // sortable as signed
    }
};

__global__ __launch_bounds__(256) void replay_compact_kernel(const uint32_t* __restrict__ okeys, int64_t count, uint32_t n,
                                                             int first, int prev_shift, int prev_width,
                                                             const SelState* __restrict__ st_prev,
                                                             SelState* __restrict__ st_next,
                                                             const uint32_t* __restrict__ hist_prev,
                                                             uint32_t* __restrict__ out_count,
                                                             int32_t* __restrict__ out_rows, float* __restrict__ out_d,
                                                             int64_t* __restrict__ out_comp) {
    const ReplayOut out{okeys, out_rows, out_d, out_comp};
    sel_compact(okeys, count, 0, n, first, prev_shift, prev_width, st_prev, st_next, hist_prev, out_count, out);
}

// the checks both entry points share; fills *dr and *sc
int replay_args(const float* meta, int64_t count, float now, int priority, float alpha, const int32_t* tags,
                int64_t n_tags, int conditions, float newer_than, float older_than, float min_strength, uint64_t seed,
                uint64_t draw, ReplayDraw* dr, ReplayScope* sc) {
    if (count < 0 || count > 0x7ffffff0LL) return AURA_E_INVAL;
    if (!(alpha >= 0.0f && alpha <= 16.0f)) return AURA_E_INVAL;                // (NaN fails both)
    if (priority != AURA_REPLAY_KEY && priority != AURA_REPLAY_STRENGTH && priority != AURA_REPLAY_UNIFORM)
        return AURA_E_INVAL;
    if (n_tags < 0 || n_tags > AURA_REPLAY_MAX_TAGS || (n_tags > 0 && !tags) || (conditions & ~7)) return AURA_E_INVAL;
    for (int64_t i = 0; i < n_tags; ++i)
        if (tags[i] < 0 || tags[i] >= (1 << 24) || (i > 0 && tags[i] <= tags[i - 1])) return AURA_E_INVAL;
    if (count > 0 && !meta) return AURA_E_INVAL;
    if (reinterpret_cast<uintptr_t>(meta) & 15) return AURA_E_ALIGN;
    dr->seed_lo = (uint32_t)seed; dr->seed_hi = (uint32_t)(seed >> 32);
    dr->draw_lo = (uint32_t)draw; dr->draw_hi = (uint32_t)(draw >> 32);
    dr->priority = priority; dr->alpha = alpha; dr->now = now;
    sc->n_tags = (int32_t)n_tags; sc->conditions = conditions;
    sc->newer_than = newer_than; sc->older_than = older_than; sc->min_strength = min_strength;
    for (int i = 0; i < AURA_REPLAY_MAX_TAGS; ++i) sc->tags[i] = i < n_tags ? tags[i] : 0x7fffffff;
    return AURA_OK;
}

}  // namespace

extern "C" {

int aura_bank_replay_keys(const float* meta, int64_t count, float now, int priority, float alpha, const int32_t* tags,
                          int64_t n_tags, int conditions, float newer_than, float older_than, float min_strength,
                          uint64_t seed, uint64_t draw, float* out_d, uint32_t* out_u, void* stream) {
    ReplayDraw dr;
    ReplayScope sc;
    const int rc = replay_args(meta, count, now, priority, alpha, tags, n_tags, conditions, newer_than, older_than,
                               min_strength, seed, draw, &dr, &sc);
    if (rc) return rc;
    if (count == 0) return AURA_OK;
    if (!out_d) return AURA_E_INVAL;
    int64_t blocks = (count + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(replay_keys_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const float4*>(meta), count, dr, sc, out_d, out_u, nullptr, nullptr, nullptr,
                       (int64_t)0, nullptr, nullptr, nullptr);
    return aura_check_launch();
}

int64_t aura_bank_replay_workspace_bytes(int64_t count, int64_t n) {
    if (count < 0 || count > 0x7ffffff0LL || n < 1) return -1;
    if (count == 0) return 0;
    if (n > count) return -1;
    return sel_workspace_bytes(count, n);
}

int aura_bank_replay(const float* meta, int64_t count, float now, int priority, float alpha, const int32_t* tags,
                     int64_t n_tags, int conditions, float newer_than, float older_than, float min_strength,
                     uint64_t seed, uint64_t draw, int64_t n, int32_t* out_rows, float* out_d, int64_t* out_eligible,
                     void* workspace, int64_t workspace_bytes, void* stream) {
    ReplayDraw dr;
    ReplayScope sc;
    int rc = replay_args(meta, count, now, priority, alpha, tags, n_tags, conditions, newer_than, older_than,
                         min_strength, seed, draw, &dr, &sc);
    if (rc) return rc;
    if (n < 1 || n > 0x7ffffff0LL || (count > 0 && n > count)) return AURA_E_INVAL;
    if (!out_rows || !out_d || !out_eligible) return AURA_E_INVAL;
    if ((reinterpret_cast<uintptr_t>(out_rows) & 3) || (reinterpret_cast<uintptr_t>(out_d) & 3) ||
        (reinterpret_cast<uintptr_t>(out_eligible) & 7))
        return AURA_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (count == 0) {                                       // the padding alone: fills, no kernel
        if (hipMemsetAsync(out_rows, 0xff, (size_t)(4 * n), s) != hipSuccess ||
            hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(out_d), (int)0xff800000u, (size_t)n, s) != hipSuccess ||
            hipMemsetAsync(out_eligible, 0, 8, s) != hipSuccess)
            return AURA_E_LAUNCH;
        return AURA_OK;
    }
    if (!workspace) return AURA_E_INVAL;
    if (reinterpret_cast<uintptr_t>(workspace) & 255) return AURA_E_ALIGN;
    if (workspace_bytes < aura_bank_replay_workspace_bytes(count, n)) return AURA_E_INVAL;
    const SelWorkspace ws = sel_workspace(workspace, n);
    if (hipMemsetAsync(ws.st, 0, (size_t)ws.clear_bytes, s) != hipSuccess ||
        hipMemsetAsync(out_eligible, 0, 8, s) != hipSuccess)
        return AURA_E_LAUNCH;
    int shifts[SEL_MAX_PASSES], widths[SEL_MAX_PASSES];
    const int P = sel_passes(count, shifts, widths);
    int64_t blocks = (count + 255) / 256;
    if (blocks > SEL_MAX_BLOCKS) blocks = SEL_MAX_BLOCKS;
    hipLaunchKernelGGL(replay_keys_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s,
                       reinterpret_cast<const float4*>(meta), count, dr, sc, out_d, nullptr, ws.okeys, ws.hist, ws.st, n,
                       out_rows, ws.out_comp, reinterpret_cast<unsigned long long*>(out_eligible));
    rc = aura_check_launch();
    if (rc) return rc;
    rc = sel_launch_passes(ws, count, 0, n, shifts, widths, P, s);
    if (rc) return rc;
    hipLaunchKernelGGL(replay_compact_kernel, dim3((unsigned)sel_blocks4(count)), dim3(256), 0, s, ws.okeys, count,
                       (uint32_t)n, P == 1 ? 1 : 0, shifts[P - 1], widths[P - 1], ws.st + (P - 1), ws.st + P,
                       ws.hist + (int64_t)(P - 1) * SEL_COPIES * SEL_BINS, &ws.st[0].out_count, out_rows, out_d,
                       ws.out_comp);
    return aura_check_launch();
}

}  // extern "C"
