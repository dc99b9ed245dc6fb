// aura_bank.hip -- maintenance kernels of the episodic bank for gfx950 (MI355X): the bf16 shadow
// rows the two-stage recall streams (plain and list-sorted, with their per-row rounding-error
// norms), incremental upkeep of the inverted lists after writes, and the centroid rebuild's means
// as a segmented reduction over rows grouped by cluster (rebuild_centroids,
// src/core/hippocampal.py:345-377), and retention: the key a full bank evicts by, the selection of its
// weakest rows and the reinforcement of recalled rows.  All HBM-bound streaming / gather kernels, no MFMA.
//
// Shadow rows.  shadow[r] = bf16(bank[r] * inv_norm[r]): the NORMALISED row rounded to bf16, so
// the prefilter's accumulator is the cosine itself.  Beside it rho[r] is an upper bound of
//     || bf16(r_hat) - r_hat_true ||_2          (r_hat_true = bank[r] / ||bank[r]||, norm 1)
// computed from the row's actual rounding residual (typically 0.0017 against the worst case
// 2^-8 = 0.0039): the data-dependent half of the two-stage recall's error bound, see
// aura_knn_coarse.inl.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/aura_hip.h"
#include "aura_common.inl"

#pragma clang fp contract(off)

namespace {

#include "aura_rowc.inl"
#include "aura_row.inl"      // shadow_convert_row: one wave converts one row and returns its rho

__device__ __forceinline__ void shadow_zero_row(uint16_t* __restrict__ dst, int64_t D, int lane) {
    for (int64_t c = lane; c < D / 8; c += 64)
        *reinterpret_cast<uint4*>(dst + 8 * c) = make_uint4(0u, 0u, 0u, 0u);
}

// shadow[r] / rho[r] for r in slots[0..n) or [row0, row0 + n); one wave per row
__global__ __launch_bounds__(256) void bank_shadow_kernel(const float* __restrict__ bank,
                                                          const float* __restrict__ inv_norm,
                                                          uint16_t* __restrict__ shadow,
                                                          float* __restrict__ rho,
                                                          const int64_t* __restrict__ slots, int64_t row0,
                                                          int64_t n, int64_t D) {
    const int lane = threadIdx.x & 63;
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += (int64_t)gridDim.x * 4) {
        const int64_t row = slots ? slots[i] : row0 + i;
        const float r = shadow_convert_row(bank + row * D, inv_norm[row], shadow + row * D, D, lane);
        if (lane == 0) rho[row] = r;
    }
}

// list-sorted shadow: sorted row i holds the shadow row of bank row sorted_rows[i] (zeros for -1);
// also refreshes rho[row] and, when given, the reverse map pos_of_row[row] = i.  F16: the image is IEEE half
// (aura_row.inl's rule); rho[row] still receives the bf16 residual, bit for bit what bank_shadow_kernel writes (the
// row-ordered shadow shares that array), and rho16[row], when given, the half image's own
template <bool F16>
__global__ __launch_bounds__(256) void bank_shadow_sorted_kernel(const float* __restrict__ bank,
                                                                 const float* __restrict__ inv_norm,
                                                                 const int32_t* __restrict__ sorted_rows,
                                                                 uint16_t* __restrict__ out,
                                                                 float* __restrict__ rho,
                                                                 float* __restrict__ rho16,
                                                                 int32_t* __restrict__ pos_of_row,
                                                                 int64_t n_sorted, int64_t D) {
    const int lane = threadIdx.x & 63;
    for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < n_sorted; i += (int64_t)gridDim.x * 4) {
        const int32_t row = sorted_rows[i];
        if (row < 0) {
            shadow_zero_row(out + i * D, D, lane);
            continue;
        }
        float r, r16 = 0.0f;
        if constexpr (F16) r16 = shadow_convert_row_f16(bank + (int64_t)row * D, inv_norm[row], out + i * D, D, lane, r);
        else r = shadow_convert_row(bank + (int64_t)row * D, inv_norm[row], out + i * D, D, lane);
        if (lane == 0) {
            rho[row] = r;
            if (F16 && rho16) rho16[row] = r16;
            if (pos_of_row) pos_of_row[row] = (int32_t)i;
        }
    }
}

// Incremental upkeep of the inverted lists after a write of n DISTINCT bank rows `slots`: the row's old
// entry (if any) becomes a hole (sorted_rows = -1: scanned as padding), and the row is appended to the
// list of its centroid id meta[slot][2] (none if < 0) inside the list's slack.  One wave per row.
// The host guarantees the slack suffices (it counts appended rows and re-packs in time); a list that is
// full nevertheless sets *flag and drops the row from the lists.  F16: a half image; rho as ever, rho16 (when given)
// the half residual; the cached constants are those of the half image and need rho16.
template <bool F16>
__global__ __launch_bounds__(256) void ivf2_append_kernel(const float* __restrict__ bank,
                                                          const float* __restrict__ inv_norm,
                                                          const float* __restrict__ meta,
                                                          const int64_t* __restrict__ slots, int64_t n,
                                                          int64_t D, uint16_t* __restrict__ sorted_bf16,
                                                          int32_t* __restrict__ sorted_rows,
                                                          const int32_t* __restrict__ pad_off,
                                                          int32_t* __restrict__ list_len,
                                                          int32_t* __restrict__ pos_of_row,
                                                          float* __restrict__ rho, float* __restrict__ rho16,
                                                          int32_t* __restrict__ flag,
                                                          float4* __restrict__ rowc, float rowc_now) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int64_t slot = slots[i];
    int pos = -1;
    if (lane == 0) {
        const int old = pos_of_row[slot];
        if (old >= 0) {
            sorted_rows[old] = -1;
            if (rowc) rowc[old] = ivf2_row_constants(-1, meta, rho, rowc_now, (float)D, F16);
        }
        const int c = (int)meta[slot * 4 + 2];
        if (c >= 0 && c < 256) {
            const int p = atomicAdd(&list_len[c], 1);
            if (p < pad_off[c + 1] - pad_off[c]) {
                pos = pad_off[c] + p;
                sorted_rows[pos] = (int32_t)slot;
            } else {
                atomicSub(&list_len[c], 1);
                atomicOr(flag, 1);
            }
        }
        pos_of_row[slot] = pos;
    }
    pos = __shfl(pos, 0);
    if (pos < 0) return;
    float r, r16 = 0.0f;
    if constexpr (F16) r16 = shadow_convert_row_f16(bank + slot * D, inv_norm[slot], sorted_bf16 + (int64_t)pos * D, D, lane, r);
    else r = shadow_convert_row(bank + slot * D, inv_norm[slot], sorted_bf16 + (int64_t)pos * D, D, lane);
    if (lane == 0) {
        rho[slot] = r;
        if (F16 && rho16) rho16[slot] = r16;
        // the caller's cached score constants (aura_ivf2_row_constants) follow the new entry
        if (rowc) {
            const float4 m = *reinterpret_cast<const float4*>(meta + slot * 4);
            const float r_img = F16 ? r16 : r;
            rowc[pos] = coarse_row_constants(m, 0.0f, &r_img, rowc_now, aura_e_fix((float)D), 0.0f,
                                             F16 ? coarse_eq_worst_f16((float)D) : coarse_eq_worst((float)D),
                                             __int_as_float((int32_t)slot));
        }
    }
}

// ------------------------------------------------------------------------------------------
// Centroid means as a segmented reduction (rebuild_centroids' masked means, hippocampal.py:358-363).
// Rows arrive grouped by cluster: order[seg_off[c] .. seg_off[c+1]) are the rows of cluster c.
// Stage 1: item = (cluster, chunk of KM_SEG consecutive rows of its segment); one wave sums its rows
//   in order (the feature dim across lanes, 16-byte loads: every row is one contiguous 4 D-byte read)
//   into partial[item][D].  Stage 2: one wave per (cluster, 256-column slice) adds the cluster's
//   partials in chunk order and divides by the count.  Fixed summation order -> reproducible means;
//   the bank is read once: N D 4 bytes + 2 N D 4 / KM_SEG of partials.
// ------------------------------------------------------------------------------------------
constexpr int KM_SEG = 64;

// s_pref[c] = first item of cluster c, s_pref[k] = number of items (k <= 256, 256 threads)
__device__ __forceinline__ void km_item_prefix(const int32_t* __restrict__ seg_off, int k, int* s_pref) {
    const int tid = threadIdx.x;
    int v = 0;
    if (tid < k) v = (seg_off[tid + 1] - seg_off[tid] + KM_SEG - 1) / KM_SEG;
    s_pref[tid + 1] = v;
    if (tid == 0) s_pref[0] = 0;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {              // inclusive scan of s_pref[1..256]
        const int add = tid >= off ? s_pref[tid + 1 - off] : 0;
        __syncthreads();
        s_pref[tid + 1] += add;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void kmeans_partial_kernel(const float* __restrict__ bank,
                                                             const int32_t* __restrict__ order,
                                                             const int32_t* __restrict__ seg_off,
                                                             float* __restrict__ partial, int64_t D, int k) {
    __shared__ int s_pref[257];
    km_item_prefix(seg_off, k, s_pref);
    const int lane = threadIdx.x & 63;
    const int n_items = s_pref[k];
    for (int item = blockIdx.x * 4 + (threadIdx.x >> 6); item < n_items; item += gridDim.x * 4) {
        int lo = 0, hi = k;                                 // cluster c with s_pref[c] <= item < s_pref[c+1]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s_pref[mid] <= item) lo = mid; else hi = mid;
        }
        const int c = lo;
        const int beg = seg_off[c] + (item - s_pref[c]) * KM_SEG;
        const int end = seg_off[c + 1];
        const int cnt = (end - beg) < KM_SEG ? (end - beg) : KM_SEG;
        const int32_t rid = lane < cnt ? order[beg + lane] : 0;
        float* const out = partial + (int64_t)item * D;
        for (int64_t col = (int64_t)lane * 4; col < D; col += 256) {
            float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, a2 = a0, a3 = a0;
            int r = 0;
            for (; r + 4 <= cnt; r += 4) {                  // four rows in flight; fixed association
                const float4 x0 = *reinterpret_cast<const float4*>(bank + (int64_t)__builtin_amdgcn_readlane(rid, r) * D + col);
                const float4 x1 = *reinterpret_cast<const float4*>(bank + (int64_t)__builtin_amdgcn_readlane(rid, r + 1) * D + col);
                const float4 x2 = *reinterpret_cast<const float4*>(bank + (int64_t)__builtin_amdgcn_readlane(rid, r + 2) * D + col);
                const float4 x3 = *reinterpret_cast<const float4*>(bank + (int64_t)__builtin_amdgcn_readlane(rid, r + 3) * D + col);
                a0.x += x0.x; a0.y += x0.y; a0.z += x0.z; a0.w += x0.w;
                a1.x += x1.x; a1.y += x1.y; a1.z += x1.z; a1.w += x1.w;
                a2.x += x2.x; a2.y += x2.y; a2.z += x2.z; a2.w += x2.w;
                a3.x += x3.x; a3.y += x3.y; a3.z += x3.z; a3.w += x3.w;
            }
            for (; r < cnt; ++r) {
                const float4 x0 = *reinterpret_cast<const float4*>(bank + (int64_t)__builtin_amdgcn_readlane(rid, r) * D + col);
                a0.x += x0.x; a0.y += x0.y; a0.z += x0.z; a0.w += x0.w;
            }
            float4 s;
            s.x = (a0.x + a1.x) + (a2.x + a3.x); s.y = (a0.y + a1.y) + (a2.y + a3.y);
            s.z = (a0.z + a1.z) + (a2.z + a3.z); s.w = (a0.w + a1.w) + (a2.w + a3.w);
            *reinterpret_cast<float4*>(out + col) = s;
        }
    }
}

__global__ __launch_bounds__(256) void kmeans_reduce_kernel(const float* __restrict__ partial,
                                                            const int32_t* __restrict__ seg_off,
                                                            float* __restrict__ centroids, int64_t D, int k,
                                                            int sums_only) {
    __shared__ int s_pref[257];
    km_item_prefix(seg_off, k, s_pref);
    const int lane = threadIdx.x & 63;
    const int slices = (int)((D + 255) / 256);
    for (int w = blockIdx.x * 4 + (threadIdx.x >> 6); w < k * slices; w += gridDim.x * 4) {
        const int c = w / slices;
        const int64_t col = (int64_t)(w - c * slices) * 256 + lane * 4;
        const int len = seg_off[c + 1] - seg_off[c];
        if (col >= D) continue;
        if (len <= 0) {                                     // empty clusters keep their centroid (:362-363);
            if (sums_only) *reinterpret_cast<float4*>(centroids + (int64_t)c * D + col) = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;                                       // as a partial sum an empty cluster is zero
        }
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int it = s_pref[c]; it < s_pref[c + 1]; ++it) {
            const float4 x = *reinterpret_cast<const float4*>(partial + (int64_t)it * D + col);
            s.x += x.x; s.y += x.y; s.z += x.z; s.w += x.w;
        }
        const float inv = sums_only ? 1.0f : (float)len;
        *reinterpret_cast<float4*>(centroids + (int64_t)c * D + col) =
            make_float4(s.x / inv, s.y / inv, s.z / inv, s.w / inv);
    }
}

// meta[i][2] = assign[i]; counts[c] = rows of cluster c (hippocampal.py:370-376)
__global__ __launch_bounds__(256) void kmeans_commit_kernel(const int32_t* __restrict__ assign,
                                                            const int32_t* __restrict__ seg_off,
                                                            float* __restrict__ meta,
                                                            float* __restrict__ counts, int64_t N, int k) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < N) meta[i * 4 + 2] = (float)assign[i];
    if (blockIdx.x == 0 && counts && (int)threadIdx.x < k)
        counts[threadIdx.x] = (float)(seg_off[threadIdx.x + 1] - seg_off[threadIdx.x]);
}

// ------------------------------------------------------------------------------------------
// Retention: which rows go first when the bank is full, and reinforcement of recalled rows.
//   key(r) = strength(r) * expf(-(now - timestamp(r)) / 3600)   -- the part of the recall score that
//   belongs to the row alone (coarse_row_constants' strength and tw, without the weight 0.2).
// Eviction order: (key, (r - cursor) mod count) ascending, NaN keys first.  As ONE 64-bit composite
//     comp(r) = ordered_u32(key(r)) << 32 | rotated_row(r)
// the first n rows of that order are the n smallest composites (all distinct: the rotated row is).
// aura_bank_select_weakest is a radix select over comp, most significant digit first (aura_select.inl, shared with the
// replay draw of aura_replay.hip): pass 0 below reads the metadata once (16 B per row), stores ordered_u32(key) (4 B per
// row) and histograms its top 12 bits; the digit passes read the 4-byte keys; the compaction writes the rows with
// comp <= threshold (exactly n of them).  A bank of equal keys (never decayed or reinforced) is seen by pass 0
// (min == max): the threshold is then the rotated row n - 1 itself and nothing but pass 0 and the compaction reads
// the rows.
// ------------------------------------------------------------------------------------------
#include "aura_retention.inl"
#include "aura_select.inl"

// out[r] = key(r)
__global__ __launch_bounds__(256) void retention_keys_kernel(const float4* __restrict__ meta, int64_t count, float now,
                                                             float* __restrict__ out) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < count; r += (int64_t)gridDim.x * 256) {
        const float4 m = meta[r];
        out[r] = retention_key(m.x, m.y, now);
    }
}

// A row whose bit is set in a caller's bitmap (aura_bank_select_weakest_masked: the tag victims of the same run) takes
// no part: pass 0 files it under an ordered key no float maps to (0xffffffff would be a positive NaN, and NaN maps to
// 0), above +inf, so the digit passes need not know of the bitmap, and the compaction leaves it out by its bit.  With
// such a row present min != max, so the equal-keys shortcut (which counts ring positions) is not taken.
constexpr uint32_t SEL_MASKED_KEY = 0xffffffffu;

__device__ __forceinline__ bool sel_masked(const uint32_t* __restrict__ bitmap, int64_t r) {
    return (bitmap[r >> 5] >> (r & 31)) & 1u;
}

// pass 0: ordered keys + histogram of their top 12 bits + min / max
template <bool MASKED>
__global__ __launch_bounds__(256) void select_keys_kernel(const float4* __restrict__ meta, int64_t count, float now,
                                                          uint32_t* __restrict__ okeys, uint32_t* __restrict__ hist,
                                                          SelState* __restrict__ st0,
                                                          const uint32_t* __restrict__ bitmap) {
    __shared__ uint32_t s_hist[SEL_BINS];
    __shared__ uint32_t s_mm[2];
    for (int b = threadIdx.x; b < SEL_BINS; b += 256) s_hist[b] = 0;
    if (threadIdx.x < 2) s_mm[threadIdx.x] = 0;
    __syncthreads();
    uint32_t kmax = 0, kmin_inv = 0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t r0 = (int64_t)blockIdx.x * 256 + threadIdx.x; r0 < count; r0 += 4 * stride) {
        float4 m[4];                                        // four 16-byte loads in flight per lane
#pragma unroll
        for (int j = 0; j < 4; ++j)
            m[j] = r0 + j * stride < count ? meta[r0 + j * stride] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t r = r0 + j * stride;
            if (r >= count) break;
            uint32_t ok = retention_ordered(retention_key(m[j].x, m[j].y, now));
            if constexpr (MASKED) {
                if (sel_masked(bitmap, r)) ok = SEL_MASKED_KEY;
            }
            okeys[r] = ok;
            kmax = max(kmax, ok); kmin_inv = max(kmin_inv, ~ok);
            sel_hist_add(s_hist, ok >> 20);
        }
    }
    sel_minmax_flush(kmax, kmin_inv, s_hist, s_mm, hist, st0);
}

// what the compaction of the retention selection writes per row: slot, key and the composite; MASKED: rows whose bit is
// set in the bitmap take no part
template <bool MASKED>
struct WeakestOut {
    const uint32_t* __restrict__ okeys;
    const float4* __restrict__ meta;
    float now;
    int64_t cursor, count;
    int64_t* __restrict__ out_slots;
    float* __restrict__ out_keys;
    int64_t* __restrict__ out_comp;
    const uint32_t* __restrict__ bitmap;
    __device__ __forceinline__ bool skip(uint32_t, int64_t r) const {
        if constexpr (MASKED) {
            if (sel_masked(bitmap, r)) return true;
        }
        return false;
    }
    __device__ __forceinline__ void write(uint32_t pos, int64_t r) const {
        const float4 m = meta[r];
        out_slots[pos] = r;
        out_keys[pos] = retention_key(m.x, m.y, now);
        out_comp[pos] = (int64_t)(retention_comp(okeys[r], r, cursor, count) ^ 0x8000000000000000ull);   // sortable as signed
    }
};

// the last narrowing, then every row at or below the threshold, in arrival order
template <bool MASKED>
__global__ __launch_bounds__(256) void select_compact_kernel(const uint32_t* __restrict__ okeys,
                                                             const float4* __restrict__ meta, int64_t count, float now,
                                                             int64_t cursor, uint32_t n, int first, int prev_shift,
                                                             int prev_width, const SelState* __restrict__ st_prev,
                                                             SelState* __restrict__ st_next,
                                                             const uint32_t* __restrict__ hist_prev,
                                                             uint32_t* __restrict__ out_count,
                                                             int64_t* __restrict__ out_slots,
                                                             float* __restrict__ out_keys,
                                                             int64_t* __restrict__ out_comp,
                                                             const uint32_t* __restrict__ bitmap) {
    const WeakestOut<MASKED> out{okeys, meta, now, cursor, count, out_slots, out_keys, out_comp, bitmap};
    sel_compact(okeys, count, cursor, n, first, prev_shift, prev_width, st_prev, st_next, hist_prev, out_count, out);
}

// meta[r][0] = min(meta[r][0] + amount, cap) where below cap, once per distinct valid r of rows[0..n_rows): the
// thread that finds the row's bit clear does the update
__global__ __launch_bounds__(256) void bank_reinforce_kernel(float* __restrict__ meta, int64_t count,
                                                             const int32_t* __restrict__ rows, int64_t n_rows,
                                                             float amount, float cap, uint32_t* __restrict__ seen) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_rows; i += (int64_t)gridDim.x * 256) {
        const int32_t r = rows[i];
        if (r < 0 || (int64_t)r >= count) continue;
        const uint32_t bit = 1u << (r & 31);
        if (atomicOr(&seen[r >> 5], bit) & bit) continue;
        const float s = meta[(int64_t)r * 4];
        if (s < cap) meta[(int64_t)r * 4] = fminf(s + amount, cap);
    }
}

}  // namespace

extern "C" {

int aura_bank_shadow_update(const float* bank, const float* inv_norm, uint16_t* bank_bf16, float* rho,
                            const int64_t* slots, int64_t row0, int64_t n, int64_t D, void* stream) {
    if (n < 0 || D <= 0 || (D & 7) || row0 < 0) return AURA_E_INVAL;
    if (n == 0) return AURA_OK;
    if (!bank || !inv_norm || !bank_bf16 || !rho) return AURA_E_INVAL;
    if ((reinterpret_cast<uintptr_t>(bank) & 15) || (reinterpret_cast<uintptr_t>(bank_bf16) & 15)) return AURA_E_ALIGN;
    int64_t blocks = (n + 3) / 4;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(bank_shadow_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       bank, inv_norm, bank_bf16, rho, slots, row0, n, D);
    return aura_check_launch();
}

// image_format with rho16: AURA_IMAGE_F16, or AURA_IMAGE_BF16 without a rho16 (the half image's residuals)
static bool bad_image_format(int image_format, const float* rho16) {
    return image_format != AURA_IMAGE_F16 && (image_format != AURA_IMAGE_BF16 || rho16);
}

int aura_bank_shadow_sorted(const float* bank, const float* inv_norm, const int32_t* sorted_rows, uint16_t* image,
                            float* rho, float* rho16, int32_t* pos_of_row, int64_t n_sorted, int64_t D,
                            int image_format, void* stream) {
    if (bad_image_format(image_format, rho16)) return AURA_E_INVAL;
    const bool f16 = image_format == AURA_IMAGE_F16;
    if (n_sorted < 0 || D <= 0 || (D & 7)) return AURA_E_INVAL;
    if (n_sorted == 0) return AURA_OK;
    if (!bank || !inv_norm || !sorted_rows || !image || !rho) return AURA_E_INVAL;
    if ((reinterpret_cast<uintptr_t>(bank) & 15) || (reinterpret_cast<uintptr_t>(image) & 15)) return AURA_E_ALIGN;
    int64_t blocks = (n_sorted + 3) / 4;
    if (blocks > 16384) blocks = 16384;
    if (f16)
        hipLaunchKernelGGL(bank_shadow_sorted_kernel<true>, dim3((unsigned)blocks), dim3(256), 0,
                           static_cast<hipStream_t>(stream), bank, inv_norm, sorted_rows, image, rho, rho16, pos_of_row,
                           n_sorted, D);
    else
        hipLaunchKernelGGL(bank_shadow_sorted_kernel<false>, dim3((unsigned)blocks), dim3(256), 0,
                           static_cast<hipStream_t>(stream), bank, inv_norm, sorted_rows, image, rho, rho16, pos_of_row,
                           n_sorted, D);
    return aura_check_launch();
}

int aura_ivf2_append(const float* bank, const float* inv_norm, const float* meta, const int64_t* slots,
                     int64_t n, int64_t D, uint16_t* image, int32_t* sorted_rows, const int32_t* pad_off,
                     int32_t* list_len, int32_t* pos_of_row, float* rho, float* rho16, int32_t* flag,
                     float* row_constants, float row_constants_now, int image_format, void* stream) {
    if (bad_image_format(image_format, rho16)) return AURA_E_INVAL;
    const bool f16 = image_format == AURA_IMAGE_F16;
    if (n < 0 || D <= 0 || (D & 7)) return AURA_E_INVAL;
    if (reinterpret_cast<uintptr_t>(row_constants) & 15) return AURA_E_ALIGN;
    if (n == 0) return AURA_OK;
    if (!bank || !inv_norm || !meta || !slots || !image || !sorted_rows || !pad_off || !list_len ||
        !pos_of_row || !rho || !flag)
        return AURA_E_INVAL;
    if (f16 && row_constants && !rho16) return AURA_E_INVAL;   // the half image's constants come from rho16
    if ((reinterpret_cast<uintptr_t>(bank) & 15) || (reinterpret_cast<uintptr_t>(image) & 15)) return AURA_E_ALIGN;
    if (f16)
        hipLaunchKernelGGL(ivf2_append_kernel<true>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), bank, inv_norm, meta, slots, n, D, image, sorted_rows,
                           pad_off, list_len, pos_of_row, rho, rho16, flag, reinterpret_cast<float4*>(row_constants),
                           row_constants_now);
    else
        hipLaunchKernelGGL(ivf2_append_kernel<false>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), bank, inv_norm, meta, slots, n, D, image, sorted_rows,
                           pad_off, list_len, pos_of_row, rho, rho16, flag, reinterpret_cast<float4*>(row_constants),
                           row_constants_now);
    return aura_check_launch();
}

int64_t aura_kmeans_means_workspace_bytes(int64_t N, int64_t D, int k) {
    if (N < 0 || D <= 0 || k <= 0 || k > 256) return -1;
    return ((N + KM_SEG - 1) / KM_SEG + k + 1) * D * 4;
}

int aura_kmeans_segment_means(const float* bank, const int32_t* order, const int32_t* seg_off, float* centroids,
                              void* workspace, int64_t workspace_bytes, int64_t N, int64_t D, int k,
                              int sums_only, void* stream) {
    if (N < 0 || N > 0x7ffffff0LL || D <= 0 || (D & 3) || k <= 0 || k > 256) return AURA_E_INVAL;
    if (N == 0) {                                           // every cluster is empty: zero sums, means keep their rows
        if (!sums_only) return AURA_OK;                     // (seg_off is not read: an empty call may pass none)
        if (!centroids) return AURA_E_INVAL;                // the caller vouches for k rows of D floats, as on the
                                                            // path below (ops.kmeans_segment_means checks the shape)
        return hipMemsetAsync(centroids, 0, (size_t)k * (size_t)D * sizeof(float), static_cast<hipStream_t>(stream)) ==
                       hipSuccess ? AURA_OK : AURA_E_LAUNCH;
    }
    if (!bank || !order || !seg_off || !centroids || !workspace) return AURA_E_INVAL;
    if ((reinterpret_cast<uintptr_t>(bank) & 15) || (reinterpret_cast<uintptr_t>(centroids) & 15) ||
        (reinterpret_cast<uintptr_t>(workspace) & 15))
        return AURA_E_ALIGN;
    if (workspace_bytes < aura_kmeans_means_workspace_bytes(N, D, k)) return AURA_E_INVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t max_items = (N + KM_SEG - 1) / KM_SEG + k;
    int64_t blocks = (max_items + 3) / 4;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(kmeans_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, s, bank, order, seg_off,
                       static_cast<float*>(workspace), D, k);
    int rc = aura_check_launch();
    if (rc) return rc;
    const int64_t waves = (int64_t)k * ((D + 255) / 256);
    hipLaunchKernelGGL(kmeans_reduce_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s,
                       static_cast<const float*>(workspace), seg_off, centroids, D, k, sums_only);
    return aura_check_launch();
}

int aura_kmeans_commit(const int32_t* assign, const int32_t* seg_off, float* meta, float* counts, int64_t N,
                       int k, void* stream) {
    if (N < 0 || k <= 0 || k > 256) return AURA_E_INVAL;
    if ((N > 0 && (!assign || !meta)) || !seg_off) return AURA_E_INVAL;   // (an empty assignment has no address)
    const int64_t blocks = N > 0 ? (N + 255) / 256 : 1;
    hipLaunchKernelGGL(kmeans_commit_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       assign, seg_off, meta, counts, N, k);
    return aura_check_launch();
}

// ---- retention ---------------------------------------------------------------------------
int aura_bank_retention_keys(const float* meta, int64_t count, float now, float* out, void* stream) {
    if (count < 0 || count > 0x7ffffff0LL) return AURA_E_INVAL;
    if (count == 0) return AURA_OK;
    if (!meta || !out) return AURA_E_INVAL;
    if (reinterpret_cast<uintptr_t>(meta) & 15) return AURA_E_ALIGN;
    int64_t blocks = (count + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(retention_keys_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const float4*>(meta), count, now, out);
    return aura_check_launch();
}

int64_t aura_bank_select_weakest_workspace_bytes(int64_t count, int64_t n) {
    if (count < 1 || count > 0x7ffffff0LL || n < 1 || n > count) return -1;
    return sel_workspace_bytes(count, n);
}

// the launches of both selections; MASKED: rows whose bit is set in `bitmap` (count bits) take no part
extern "C++" {
template <bool MASKED>
static int select_weakest_launch(const float* meta, int64_t count, float now, int64_t cursor, int64_t n,
                                 const uint32_t* bitmap, int64_t* out_slots, float* out_keys, void* workspace,
                                 int64_t workspace_bytes, void* stream) {
    if (count < 1 || count > 0x7ffffff0LL || n < 1 || n > count || cursor < 0) return AURA_E_INVAL;
    if (!meta || !out_slots || !out_keys || !workspace || (MASKED && !bitmap)) return AURA_E_INVAL;
    if ((reinterpret_cast<uintptr_t>(meta) & 15) || (reinterpret_cast<uintptr_t>(workspace) & 255)) return AURA_E_ALIGN;
    if (MASKED && (reinterpret_cast<uintptr_t>(bitmap) & 3)) return AURA_E_ALIGN;
    if (workspace_bytes < aura_bank_select_weakest_workspace_bytes(count, n)) return AURA_E_INVAL;
    cursor %= count;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const SelWorkspace ws = sel_workspace(workspace, n);
    if (hipMemsetAsync(ws.st, 0, (size_t)ws.clear_bytes, s) != hipSuccess) return AURA_E_LAUNCH;
    int shifts[SEL_MAX_PASSES], widths[SEL_MAX_PASSES];
    const int P = sel_passes(count, shifts, widths);
    const float4* meta4 = reinterpret_cast<const float4*>(meta);
    int64_t blocks = (count + 255) / 256;
    if (blocks > SEL_MAX_BLOCKS) blocks = SEL_MAX_BLOCKS;
    hipLaunchKernelGGL(select_keys_kernel<MASKED>, dim3((unsigned)blocks), dim3(256), 0, s, meta4, count, now, ws.okeys,
                       ws.hist, ws.st, bitmap);
    int rc = aura_check_launch();
    if (rc) return rc;
    rc = sel_launch_passes(ws, count, cursor, n, shifts, widths, P, s);
    if (rc) return rc;
    hipLaunchKernelGGL(select_compact_kernel<MASKED>, dim3((unsigned)sel_blocks4(count)), dim3(256), 0, s, ws.okeys, meta4,
                       count, now, cursor, (uint32_t)n, P == 1 ? 1 : 0, shifts[P - 1], widths[P - 1], ws.st + (P - 1),
                       ws.st + P, ws.hist + (int64_t)(P - 1) * SEL_COPIES * SEL_BINS, &ws.st[0].out_count, out_slots,
                       out_keys, ws.out_comp, bitmap);
    return aura_check_launch();
}
}  // extern "C++"

int aura_bank_select_weakest(const float* meta, int64_t count, float now, int64_t cursor, int64_t n,
                             int64_t* out_slots, float* out_keys, void* workspace, int64_t workspace_bytes,
                             void* stream) {
    return select_weakest_launch<false>(meta, count, now, cursor, n, nullptr, out_slots, out_keys, workspace,
                                        workspace_bytes, stream);
}

int64_t aura_bank_select_weakest_masked_workspace_bytes(int64_t count, int64_t n) {
    return aura_bank_select_weakest_workspace_bytes(count, n);
}

int aura_bank_select_weakest_masked(const float* meta, int64_t count, float now, int64_t cursor, int64_t n,
                                    const uint32_t* bitmap, int64_t* out_slots, float* out_keys, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
    return select_weakest_launch<true>(meta, count, now, cursor, n, bitmap, out_slots, out_keys, workspace,
                                       workspace_bytes, stream);
}

int64_t aura_bank_reinforce_workspace_bytes(int64_t count) {
    if (count < 0 || count > 0x7ffffff0LL) return -1;
    return aura_align256((count + 31) / 32 * 4);
}

int aura_bank_reinforce(float* meta, int64_t count, const int32_t* rows, int64_t n_rows, float amount, float cap,
                        void* workspace, int64_t workspace_bytes, void* stream) {
    if (count < 0 || count > 0x7ffffff0LL || n_rows < 0 || !(amount >= 0.0f) || cap != cap) return AURA_E_INVAL;
    if (count == 0 || n_rows == 0) return AURA_OK;
    if (!meta || !rows || !workspace) return AURA_E_INVAL;
    if (reinterpret_cast<uintptr_t>(workspace) & 3) return AURA_E_ALIGN;
    const int64_t need = aura_bank_reinforce_workspace_bytes(count);
    if (workspace_bytes < need) return AURA_E_INVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(workspace, 0, (size_t)need, s) != hipSuccess) return AURA_E_LAUNCH;
    int64_t blocks = (n_rows + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(bank_reinforce_kernel, dim3((unsigned)blocks), dim3(256), 0, s, meta, count, rows, n_rows, amount,
                       cap, static_cast<uint32_t*>(workspace));
    return aura_check_launch();
}

}  // extern "C"
