// aura_quota.hip -- per-tag quotas: how many rows every tag of a run holds, and each tag's own weakest rows; gfx950.
// [build-side] no upstream counterpart.  The rule is stated once, in include/aura_hip.h ("Per-tag quotas").
//
// aura_bank_tag_counts: one pass over the metadata; a row's tag (column 3) is looked up among the call's scope tags
// (ascending, in LDS) by binary search, counted in LDS, and every workgroup adds each non-empty scope to the result once.
//
// aura_bank_select_weakest_scoped: the radix select of aura_bank.hip with up to 64 thresholds at once.  Scope s orders
// ITS rows by  comp_s(r) = ordered_u32(key(r)) << 32 | (r - origin[s]) mod count  and takes the x_s smallest.
//   keys      reads the metadata once (16 B per row), stores (scope index, ordered key) per row (8 B) and histograms the
//             top 8 bits of the key per scope: hist[S][256], 64 KB of LDS at S = 64 (hence 8-bit digits, not 12)
//   resolve   one workgroup per scope, thread b owns bin b: the first one turns the histogram's total into held_s and
//             x_s = min(incoming, max(0, held + incoming - quota)), pads the scope's output range, and every one narrows
//             the scope's prefix by one digit (the scan of aura_bank.hip's sel_resolve, on 256 bins)
//   pass      reads the 8-byte records; histograms the next digit of the rows that match their scope's prefix.  Digits:
//             4 x 8 bits of the key, then the bits of the rotated row that `count` needs, 8 at a time
//   compact   rows with comp_s <= the scope's threshold (exactly x_s per scope): a workgroup lists its rows in LDS, counts
//             them per scope there and reserves each scope's output range with ONE global add; sets the rows' bitmap bits
// A scope whose chosen bin holds exactly the rows still needed is done early; once every scope is done the remaining
// passes return after reading the 64 states.  As in aura_bank.hip the grid is capped at 512 workgroups and the global
// histograms are kept in 4 copies (same-address adds: DESIGN 4.4).  Every atomic is an integer add or an integer or: no
// result depends on arrival order except the order of a scope's output range, which the composites written beside the
// rows resolve.  Every index is checked before it becomes an address.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/aura_hip.h"
#include "aura_common.inl"

#pragma clang fp contract(off)

namespace {

#include "aura_retention.inl"

constexpr int Q_MAX_SCOPES = AURA_QUOTA_MAX_SCOPES;
constexpr int Q_BINS = 256;             // 8-bit digits
constexpr int Q_MAX_PASSES = 8;         // 4 digits of the key + at most 4 of a 31-bit rotated row
constexpr int Q_MAX_BLOCKS = 512;
constexpr int Q_COPIES = 4;             // copies of every global histogram
constexpr int Q_LIST = 2048;            // selected rows a workgroup of the compaction holds before it writes them out
constexpr uint32_t Q_NO_SCOPE = 0xffffffffu;

static_assert(Q_MAX_SCOPES == 64, "the LDS histograms are sized for 64 scopes");

struct QState {                         // one per scope, narrowed in place by the resolve launches
    unsigned long long prefix;          // decided high bits of the threshold; the threshold itself once done
    uint32_t need;                      // rows still to take among those that match the prefix
    uint32_t done;
    uint32_t none;                      // x == 0: the scope selects nothing
    uint32_t held, x;                   // rows of [0, count) that carry the tag; victims
    uint32_t off;                       // first entry of the scope's output range
};

// index of `w` (metadata column 3 as stored) among the ascending scope tags, or -1
__device__ __forceinline__ int q_scope(float w, const int* s_tags, int S) {
    const int tag = aura_row_tag(w);
    if (tag == aura_no_tag) return -1;
    int lo = 0, hi = S;                 // first index whose tag is >= tag
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_tags[mid] < tag) lo = mid + 1; else hi = mid;
    }
    return (lo < S && s_tags[lo] == tag) ? lo : -1;
}

__device__ __forceinline__ void q_flush_hist(const uint32_t* s_hist, int S, uint32_t* __restrict__ hist) {
    hist += (blockIdx.x % Q_COPIES) * (Q_MAX_SCOPES * Q_BINS);
    for (int b = threadIdx.x; b < S * Q_BINS; b += 256) {
        const uint32_t c = s_hist[b];
        if (c) atomicAdd(&hist[b], c);
    }
}

__global__ __launch_bounds__(256) void q_tag_counts_kernel(const float* __restrict__ meta, int64_t count,
                                                           const int32_t* __restrict__ scope_tags, int S,
                                                           uint32_t* __restrict__ out) {
    __shared__ int s_tags[Q_MAX_SCOPES];
    __shared__ uint32_t s_cnt[Q_MAX_SCOPES];
    if ((int)threadIdx.x < Q_MAX_SCOPES) {
        s_tags[threadIdx.x] = (int)threadIdx.x < S ? scope_tags[threadIdx.x] : 0x7fffffff;
        s_cnt[threadIdx.x] = 0;
    }
    __syncthreads();
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < count; r += (int64_t)gridDim.x * 256) {
        const int s = q_scope(meta[r * 4 + 3], s_tags, S);
        if (s >= 0) atomicAdd(&s_cnt[s], 1u);
    }
    __syncthreads();
    if ((int)threadIdx.x < S && s_cnt[threadIdx.x]) atomicAdd(&out[threadIdx.x], s_cnt[threadIdx.x]);
}

// keys: (scope, ordered key) per row + per-scope histogram of the key's top 8 bits
__global__ __launch_bounds__(256) void q_keys_kernel(const float4* __restrict__ meta, int64_t count, float now,
                                                     const int32_t* __restrict__ scope_tags, int S,
                                                     uint2* __restrict__ rec, uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_hist[Q_MAX_SCOPES * Q_BINS];
    __shared__ int s_tags[Q_MAX_SCOPES];
    for (int b = threadIdx.x; b < S * Q_BINS; b += 256) s_hist[b] = 0;
    if ((int)threadIdx.x < Q_MAX_SCOPES) s_tags[threadIdx.x] = (int)threadIdx.x < S ? scope_tags[threadIdx.x] : 0x7fffffff;
    __syncthreads();
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < count; r += (int64_t)gridDim.x * 256) {
        const float4 m = meta[r];
        const int s = q_scope(m.w, s_tags, S);
        const uint32_t ok = retention_ordered(retention_key(m.x, m.y, now));
        rec[r] = make_uint2(s < 0 ? Q_NO_SCOPE : (uint32_t)s, ok);
        if (s >= 0) atomicAdd(&s_hist[s * Q_BINS + (ok >> 24)], 1u);
    }
    __syncthreads();
    q_flush_hist(s_hist, S, hist);
}

// One workgroup per scope.  `first`: the histogram is that of the key's top digit over ALL the scope's rows, so its total
// is held_s; x_s, the scope's output range and its padding follow.  Then the prefix takes the digit at `shift`.
__global__ __launch_bounds__(256) void q_resolve_kernel(QState* __restrict__ st, const uint32_t* __restrict__ hist,
                                                        int first, int last, int shift, int width,
                                                        const int32_t* __restrict__ incoming,
                                                        const int32_t* __restrict__ quota, int S, int64_t out_cap,
                                                        int64_t* __restrict__ out_held, int64_t* __restrict__ out_x,
                                                        int64_t* __restrict__ out_slots, int64_t* __restrict__ out_comp) {
    __shared__ uint32_t s_scan[256];
    __shared__ QState s_st;
    const int s = blockIdx.x, tid = threadIdx.x;
    if (s >= S) return;
    uint32_t c = 0;
    if (tid < (1 << width)) {
#pragma unroll
        for (int j = 0; j < Q_COPIES; ++j) c += hist[j * (Q_MAX_SCOPES * Q_BINS) + s * Q_BINS + tid];
    }
    s_scan[tid] = c;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {               // inclusive scan
        const uint32_t add = tid >= off ? s_scan[tid - off] : 0u;
        __syncthreads();
        s_scan[tid] += add;
        __syncthreads();
    }
    const uint32_t total = s_scan[255];
    if (tid == 0) {
        QState cur;
        if (first) {
            int64_t off = 0;
            for (int j = 0; j < s; ++j) off += incoming[j] > 0 ? incoming[j] : 0;
            int64_t in = incoming[s] > 0 ? incoming[s] : 0;
            if (off > out_cap) off = out_cap;
            if (off + in > out_cap) in = out_cap - off;      // (the host sized the output: cannot happen)
            const int64_t q = quota[s] > 0 ? quota[s] : 0;
            int64_t x = (int64_t)total + in - q;
            if (x < 0) x = 0;
            if (x > in) x = in;
            if (x > (int64_t)total) x = total;
            cur.prefix = x && x == (int64_t)total ? ~0ull : 0ull;   // every row of the scope
            cur.need = (uint32_t)x;
            cur.none = x == 0;
            cur.done = x == 0 || x == (int64_t)total;
            cur.held = total; cur.x = (uint32_t)x; cur.off = (uint32_t)off;
            out_held[s] = total; out_x[s] = x;
        } else {
            cur = st[s];
            if (!cur.done && total < cur.need) { cur.done = 1; cur.none = 1; }   // (a histogram short of `need`: nothing)
        }
        s_st = cur;
    }
    __syncthreads();
    QState cur = s_st;
    if (first) {                                            // unfilled entries: no row, sorted last
        const int64_t in = incoming[s] > 0 ? incoming[s] : 0;
        for (int64_t i = tid; i < in; i += 256) {
            const int64_t pos = (int64_t)cur.off + i;
            if (pos >= out_cap) break;
            out_slots[pos] = -1;
            out_comp[pos] = 0x7fffffffffffffffLL;
        }
    }
    if (!cur.done) {
        const uint32_t incl = s_scan[tid], excl = incl - c;
        if (excl < cur.need && cur.need <= incl) {          // exactly one thread: its bin holds the threshold
            const uint32_t need = cur.need - excl;
            unsigned long long prefix = cur.prefix | ((unsigned long long)tid << shift);
            const bool done = c == need || last;
            if (done && shift) prefix |= (1ull << shift) - 1ull;      // every row of the bin
            cur.prefix = prefix; cur.need = need; cur.done = done ? 1u : 0u;
            st[s] = cur;
        }
    } else if (tid == 0) {
        st[s] = cur;
    }
}

// the scopes' states and origins in LDS; returns whether any scope still narrows
__device__ __forceinline__ bool q_load_states(const QState* __restrict__ st, const int32_t* __restrict__ origin, int S,
                                              int64_t count, unsigned long long* s_prefix, uint32_t* s_flag,
                                              int32_t* s_origin, uint32_t* s_any, bool want_done) {
    if (threadIdx.x == 0) *s_any = 0;
    __syncthreads();
    if ((int)threadIdx.x < Q_MAX_SCOPES) {
        const int s = threadIdx.x;
        unsigned long long p = 0;
        uint32_t f = 0;
        int32_t o = 0;
        if (s < S) {
            const QState q = st[s];
            p = q.prefix;
            f = want_done ? (q.done && !q.none) : !q.done;    // compaction: scopes that select; pass: scopes that narrow
            int64_t oo = (int64_t)origin[s] % count;
            if (oo < 0) oo += count;
            o = (int32_t)oo;
            if (f) atomicOr(s_any, 1u);
        }
        s_prefix[s] = p; s_flag[s] = f; s_origin[s] = o;
    }
    __syncthreads();
    return *s_any != 0;
}

__global__ __launch_bounds__(256) void q_pass_kernel(const uint2* __restrict__ rec, int64_t count,
                                                     const QState* __restrict__ st, const int32_t* __restrict__ origin,
                                                     int S, int prev_shift, int shift, int width,
                                                     uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_hist[Q_MAX_SCOPES * Q_BINS];
    __shared__ unsigned long long s_prefix[Q_MAX_SCOPES];
    __shared__ uint32_t s_active[Q_MAX_SCOPES];
    __shared__ int32_t s_origin[Q_MAX_SCOPES];
    __shared__ uint32_t s_any;
    if (!q_load_states(st, origin, S, count, s_prefix, s_active, s_origin, &s_any, false)) return;   // (uniform)
    for (int b = threadIdx.x; b < S * Q_BINS; b += 256) s_hist[b] = 0;
    __syncthreads();
    const uint32_t mask = (1u << width) - 1u;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < count; r += (int64_t)gridDim.x * 256) {
        const uint2 v = rec[r];
        if (v.x >= (uint32_t)S || !s_active[v.x]) continue;
        const uint64_t comp = retention_comp(v.y, r, s_origin[v.x], count);
        if ((comp >> prev_shift) == (s_prefix[v.x] >> prev_shift))
            atomicAdd(&s_hist[v.x * Q_BINS + ((uint32_t)(comp >> shift) & mask)], 1u);
    }
    __syncthreads();
    q_flush_hist(s_hist, S, hist);
}

__global__ __launch_bounds__(256) void q_compact_kernel(const uint2* __restrict__ rec, int64_t count,
                                                        const QState* __restrict__ st,
                                                        const int32_t* __restrict__ origin, int S, int64_t out_cap,
                                                        uint32_t* __restrict__ out_count,
                                                        int64_t* __restrict__ out_slots, int64_t* __restrict__ out_comp,
                                                        uint32_t* __restrict__ bitmap) {
    __shared__ unsigned long long s_thr[Q_MAX_SCOPES];
    __shared__ uint32_t s_sel[Q_MAX_SCOPES];
    __shared__ int32_t s_origin[Q_MAX_SCOPES];
    __shared__ uint32_t s_x[Q_MAX_SCOPES], s_off[Q_MAX_SCOPES], s_cnt[Q_MAX_SCOPES], s_base[Q_MAX_SCOPES];
    __shared__ int32_t s_rows[Q_LIST];
    __shared__ uint32_t s_where[Q_LIST];                    // scope << 16 | index among the workgroup's rows of the scope
    __shared__ uint32_t s_any, s_n;
    if (!q_load_states(st, origin, S, count, s_thr, s_sel, s_origin, &s_any, true)) return;          // (uniform)
    if ((int)threadIdx.x < Q_MAX_SCOPES) {
        const bool in = (int)threadIdx.x < S;
        s_x[threadIdx.x] = in ? st[threadIdx.x].x : 0u;
        s_off[threadIdx.x] = in ? st[threadIdx.x].off : 0u;
    }
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();

    auto write_list = [&]() {
        const uint32_t cnt = s_n;
        if ((int)threadIdx.x < Q_MAX_SCOPES) s_cnt[threadIdx.x] = 0;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < cnt; i += 256) {
            const uint32_t s = s_where[i];
            s_where[i] = (s << 16) | atomicAdd(&s_cnt[s], 1u);        // (< Q_LIST <= 2^16 rows per list)
        }
        __syncthreads();
        if ((int)threadIdx.x < S && s_cnt[threadIdx.x])              // one global add per non-empty scope
            s_base[threadIdx.x] = atomicAdd(&out_count[threadIdx.x], s_cnt[threadIdx.x]);
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < cnt; i += 256) {
            const uint32_t s = s_where[i] >> 16;
            const uint32_t k = s_base[s] + (s_where[i] & 0xffffu);
            const int64_t r = s_rows[i];
            const int64_t pos = (int64_t)s_off[s] + k;
            if (k >= s_x[s] || pos >= out_cap) continue;    // (cannot happen: exactly x composites are <= the threshold)
            out_slots[pos] = r;
            out_comp[pos] = (int64_t)(retention_comp(rec[r].y, r, s_origin[s], count) ^ 0x8000000000000000ull);
            atomicOr(&bitmap[r >> 5], 1u << (r & 31));
        }
        __syncthreads();
        if (threadIdx.x == 0) s_n = 0;
        __syncthreads();
    };

    // every thread of the workgroup makes the same number of trips (barriers inside); a trip adds at most 256 rows
    for (int64_t r0 = (int64_t)blockIdx.x * 256; r0 < count; r0 += (int64_t)gridDim.x * 256) {
        const int64_t r = r0 + threadIdx.x;
        if (r < count) {
            const uint2 v = rec[r];
            if (v.x < (uint32_t)S && s_sel[v.x] && retention_comp(v.y, r, s_origin[v.x], count) <= s_thr[v.x]) {
                const uint32_t i = atomicAdd(&s_n, 1u);
                s_rows[i] = (int32_t)r;
                s_where[i] = v.x;
            }
        }
        __syncthreads();
        const uint32_t held = s_n;                          // (read by all before anyone adds again)
        __syncthreads();
        if (held > Q_LIST - 256) write_list();              // (uniform) no room for another trip
    }
    write_list();
}

// digits of the composite: four of the key, then the bits of the rotated row that `count` needs
int q_passes(int64_t count, int* shifts, int* widths) {
    int P = 0;
    for (int sh = 56; sh >= 32; sh -= 8) { shifts[P] = sh; widths[P++] = 8; }
    int s = 0;
    while (s < 31 && (1LL << s) < count) ++s;               // rotated rows are < count <= 2^s
    while (s > 0) {
        const int w = s < 8 ? s : 8;
        s -= w;
        shifts[P] = s; widths[P++] = w;
    }
    return P;
}

constexpr int64_t Q_HIST_BYTES = (int64_t)Q_COPIES * Q_MAX_SCOPES * Q_BINS * 4;   // one pass

}  // namespace

extern "C" {

int aura_bank_tag_counts(const float* meta, int64_t count, const int32_t* scope_tags, int64_t n_scopes, int32_t* out,
                         void* stream) {
    if (count < 0 || count > 0x7ffffff0LL || n_scopes < 1 || n_scopes > Q_MAX_SCOPES) return AURA_E_INVAL;
    if (!scope_tags || !out || (count > 0 && !meta)) return AURA_E_INVAL;
    if ((reinterpret_cast<uintptr_t>(meta) & 15) || (reinterpret_cast<uintptr_t>(out) & 3)) return AURA_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(out, 0, (size_t)n_scopes * 4, s) != hipSuccess) return AURA_E_LAUNCH;
    if (count == 0) return AURA_OK;
    int64_t blocks = (count + 255) / 256;
    if (blocks > Q_MAX_BLOCKS) blocks = Q_MAX_BLOCKS;
    hipLaunchKernelGGL(q_tag_counts_kernel, dim3((unsigned)blocks), dim3(256), 0, s, meta, count, scope_tags,
                       (int)n_scopes, reinterpret_cast<uint32_t*>(out));
    return aura_check_launch();
}

// workspace: [QState x 64] [64 output cursors] [histograms x passes] [records (8 B x count)]
int64_t aura_bank_select_weakest_scoped_workspace_bytes(int64_t count, int64_t n_scopes) {
    if (count < 1 || count > 0x7ffffff0LL || n_scopes < 1 || n_scopes > Q_MAX_SCOPES) return -1;
    return aura_align256(Q_MAX_SCOPES * (int64_t)sizeof(QState)) + aura_align256(Q_MAX_SCOPES * 4) + Q_MAX_PASSES * Q_HIST_BYTES +
           aura_align256(8 * count);
}

int aura_bank_select_weakest_scoped(const float* meta, int64_t count, float now, const int32_t* scope_tags,
                                    const int32_t* origin, const int32_t* incoming, const int32_t* quota,
                                    int64_t n_scopes, int64_t out_capacity, int64_t* out_held, int64_t* out_x,
                                    int64_t* out_slots, int64_t* out_comp, uint32_t* bitmap, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
    if (count < 1 || count > 0x7ffffff0LL || n_scopes < 1 || n_scopes > Q_MAX_SCOPES) return AURA_E_INVAL;
    if (out_capacity < 0 || out_capacity > 0x7ffffff0LL) return AURA_E_INVAL;
    if (!meta || !scope_tags || !origin || !incoming || !quota || !out_held || !out_x || !bitmap || !workspace)
        return AURA_E_INVAL;
    if (out_capacity > 0 && (!out_slots || !out_comp)) return AURA_E_INVAL;
    if ((reinterpret_cast<uintptr_t>(meta) & 15) || (reinterpret_cast<uintptr_t>(workspace) & 255) ||
        (reinterpret_cast<uintptr_t>(bitmap) & 3) || (reinterpret_cast<uintptr_t>(out_held) & 7) ||
        (reinterpret_cast<uintptr_t>(out_x) & 7) || (reinterpret_cast<uintptr_t>(out_slots) & 7) ||
        (reinterpret_cast<uintptr_t>(out_comp) & 7))
        return AURA_E_ALIGN;
    if (workspace_bytes < aura_bank_select_weakest_scoped_workspace_bytes(count, n_scopes)) return AURA_E_INVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int S = (int)n_scopes;
    char* w = static_cast<char*>(workspace);
    QState* st = reinterpret_cast<QState*>(w);
    w += aura_align256(Q_MAX_SCOPES * (int64_t)sizeof(QState));
    uint32_t* out_count = reinterpret_cast<uint32_t*>(w);
    w += aura_align256(Q_MAX_SCOPES * 4);
    uint32_t* hist = reinterpret_cast<uint32_t*>(w);
    w += Q_MAX_PASSES * Q_HIST_BYTES;
    uint2* rec = reinterpret_cast<uint2*>(w);
    int shifts[Q_MAX_PASSES], widths[Q_MAX_PASSES];
    const int P = q_passes(count, shifts, widths);
    if (hipMemsetAsync(workspace, 0, (size_t)(reinterpret_cast<char*>(hist) - static_cast<char*>(workspace)) +
                                         (size_t)P * Q_HIST_BYTES, s) != hipSuccess)
        return AURA_E_LAUNCH;
    int64_t blocks = (count + 255) / 256;
    if (blocks > Q_MAX_BLOCKS) blocks = Q_MAX_BLOCKS;
    const dim3 grid((unsigned)blocks), wg(256);
    hipLaunchKernelGGL(q_keys_kernel, grid, wg, 0, s, reinterpret_cast<const float4*>(meta), count, now, scope_tags, S, rec,
                       hist);
    int rc = aura_check_launch();
    if (rc) return rc;
    for (int i = 0; i < P; ++i) {
        uint32_t* h = hist + (int64_t)i * (Q_HIST_BYTES / 4);
        if (i > 0) {
            hipLaunchKernelGGL(q_pass_kernel, grid, wg, 0, s, rec, count, st, origin, S, shifts[i - 1], shifts[i], widths[i],
                               h);
            rc = aura_check_launch();
            if (rc) return rc;
        }
        hipLaunchKernelGGL(q_resolve_kernel, dim3((unsigned)S), wg, 0, s, st, h, i == 0 ? 1 : 0, i == P - 1 ? 1 : 0,
                           shifts[i], widths[i], incoming, quota, S, out_capacity, out_held, out_x, out_slots, out_comp);
        rc = aura_check_launch();
        if (rc) return rc;
    }
    hipLaunchKernelGGL(q_compact_kernel, grid, wg, 0, s, rec, count, st, origin, S, out_capacity, out_count, out_slots,
                       out_comp, bitmap);
    return aura_check_launch();
}

}  // extern "C"
