// aura_sample.hip -- the next token of every row: repetition penalty, temperature, exact top-k, nucleus and a seeded
// Gumbel-max draw in one launch, the row's generation state (seen mask, finished flag, token column) on the device
// (gfx950).
// The rule is stated once, in include/aura_hip.h ("Next token"); the comments here are about how it is computed.
//   rows        one workgroup of 1024 lanes owns a row from its logits to its state.  B is small in generation, so most
//               of the chip idles: accepted for this version.
//   keys        pass 0 reads the logits and the mask once, applies steps 1, 2 and 4 and writes every token's monotone
//               32-bit key (the float's bits with the sign folded, -0 as +0) to the workspace; the later passes read
//               the keys back (from L2: a row is at most 512 KB), so no pass repeats a division.
//   selection   the exact k'-th largest key T by a radix selection over the digits 11 / 11 / 10 bits, high to low, with an
//               integer LDS histogram per pass (bins reversed, so that an ascending prefix sum counts from the top).
//               Integer LDS atomics only: the counts do not depend on the order of arrival.
//   compaction  keys above T, and of the keys equal to T the first k' - #(above) in id order, go to an LDS list.  Each
//               wave owns a contiguous range of ids; counts per wave, a prefix over the 16 waves, then ballot prefixes
//               give every candidate a fixed position: no atomics, the list does not depend on timing.
//   order       the composites  ~key << 32 | id  are distinct; lane j counts the composites below its own and drops it
//               at that rank (k'^2 broadcast LDS reads in all, at most 1024 per lane).
//   nucleus     lane j owns rank j: expf, the blocked prefix sum of the rule (64 lanes x 16 ranks, then one lane over
//               the 64 bases), the kept test against fl(top_p S).
//   draw        Philox and two logf per kept rank only; the argmax of (d, lower id) by a wave butterfly on 64-bit
//               composites and one pass over the 16 wave results.
// The greedy and the full-vocabulary kernels are pass 0 followed by the same argmax.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "../../include/aura_hip.h"
#include "aura_common.inl"

namespace {

constexpr int SAMPLE_THREADS = 1024;
constexpr int SAMPLE_WAVES = SAMPLE_THREADS / 64;
constexpr int SAMPLE_BINS = 2048;
constexpr int SAMPLE_BLOCK = 16;            // ranks per block of the prefix sum
constexpr int SAMPLE_NBLOCKS = AURA_SAMPLE_MAX_K / SAMPLE_BLOCK;

struct SampleArgs {
    const float* logits;                // row b at logits + b * row_stride
    int64_t row_stride;
    uint8_t* seen;                      // [B][V] or NULL
    uint8_t* finished;                  // [B] or NULL
    const int64_t* streams;             // [B] or NULL
    int64_t* tokens;                    // row b at tokens + b * token_stride
    int64_t token_stride;
    int32_t* cand_ids;                  // [B][k] or NULL
    float* cand_z;
    float* cand_cum;
    float* cand_d;                      // [B][k], or [B][V] in the full-vocabulary kernel
    int32_t* n_kept;                    // [B] or NULL
    uint32_t* keys;                     // workspace [B][V]
    int V, k;                           // k = k' = min(top_k, V)
    int rule;
    float penalty, temperature, top_p;
    uint32_t seed_lo, seed_hi, step_lo, step_hi;
    int64_t eos_id, pad_id;
};

// word 0 of Philox4x32-10, counter (c0, c1, c2, c3), key (k0, k1): the constants of the replay rule
__device__ __forceinline__ uint32_t sample_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
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

// unsigned order of the keys = value order; -0 is +0; no NaN reaches it (-inf is 0x007fffff, the smallest key of a row,
// and 0 is below every key)
__device__ __forceinline__ uint32_t sample_key(float z) {
    uint32_t u = __float_as_uint(z);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sample_unkey(uint32_t key) {
    return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

// steps 1, 2 and (TEMPER) 4 of the rule for one logit
template <bool TEMPER>
__device__ __forceinline__ float sample_value(float z, bool seen, const SampleArgs& a) {
    if (z != z) z = -__builtin_inff();
    if (z > FLT_MAX) z = FLT_MAX;
    if (seen && a.penalty != 1.0f) {
        z = (a.rule == AURA_PENALTY_SIGNED && z < 0.0f) ? z * a.penalty : z / a.penalty;
        if (z > FLT_MAX) z = FLT_MAX;
    }
    if (TEMPER) {
        z = z / a.temperature;
        if (z > FLT_MAX) z = FLT_MAX;
    }
    return z;
}

// d of step 7 for token id with value z
__device__ __forceinline__ float sample_draw_key(float z, uint32_t id, uint32_t stream, const SampleArgs& a) {
    const uint32_t x = sample_philox(id, stream, a.step_lo, a.step_hi, a.seed_lo, a.seed_hi);
    const float u = ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-7f;          // 2^-23: exact
    return z + (-logf(-logf(u)));
}

__device__ __forceinline__ uint64_t sample_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ int sample_prefix(uint64_t m) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// the largest composite of the workgroup, in every lane (0: no lane offered one).  s_red: 16 words of LDS.
__device__ __forceinline__ uint64_t sample_block_max(uint64_t v, uint64_t* s_red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = __shfl_xor((unsigned long long)v, off);
        v = o > v ? o : v;
    }
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t best = 0;
#pragma unroll
    for (int w = 0; w < SAMPLE_WAVES; ++w) best = s_red[w] > best ? s_red[w] : best;
    __syncthreads();                                                    // s_red may be used again
    return best;
}

// larger value first, then the lower id: the composite whose maximum is the argmax of the rule (value never NaN)
__device__ __forceinline__ uint64_t sample_argmax_comp(float v, uint32_t id) {
    return ((uint64_t)sample_key(v) << 32) | (uint64_t)(0xffffffffu - id);
}

// the row's state, by one lane: the token, its mask byte, the finished flag
__device__ __forceinline__ void sample_write_state(const SampleArgs& a, int64_t b, int64_t token) {
    a.tokens[b * a.token_stride] = token;
    if (token < 0) return;
    if (a.seen) a.seen[b * a.V + token] = 1;
    if (a.finished && a.eos_id >= 0 && token == a.eos_id) a.finished[b] = 1;
}

// a finished row: the padding and nothing else (uniform over the workgroup)
__device__ __forceinline__ bool sample_row_finished(const SampleArgs& a, int64_t b) {
    if (!a.finished || a.finished[b] == 0) return false;
    if (threadIdx.x == 0) a.tokens[b * a.token_stride] = a.pad_id;
    return true;
}

// GREEDY: the argmax of the penalised z.  Otherwise the full-vocabulary draw: the argmax of d over the tokens with
// z > -inf, d to cand_d [B][V] when asked for.
template <bool GREEDY>
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_argmax_kernel(const SampleArgs a) {
    __shared__ uint64_t s_red[SAMPLE_WAVES];
    const int64_t b = blockIdx.x;
    if (sample_row_finished(a, b)) return;
    const float* const zr = a.logits + b * a.row_stride;
    const uint8_t* const sr = a.seen ? a.seen + b * a.V : nullptr;
    const uint32_t stream = a.streams ? (uint32_t)a.streams[b] : (uint32_t)b;
    uint64_t best = 0;
    for (int i = threadIdx.x; i < a.V; i += SAMPLE_THREADS) {
        const float z = sample_value<!GREEDY>(zr[i], sr && sr[i] != 0, a);
        const bool live = z > -__builtin_inff();
        float v = z;
        if (!GREEDY) {
            v = live ? sample_draw_key(z, (uint32_t)i, stream, a) : -__builtin_inff();
            if (a.cand_d) a.cand_d[b * a.V + i] = v;
        }
        if (live) {
            const uint64_t c = sample_argmax_comp(v, (uint32_t)i);
            best = c > best ? c : best;
        }
    }
    best = sample_block_max(best, s_red);                               // (its barriers: every lane has read the mask)
    if (threadIdx.x == 0) sample_write_state(a, b, best ? (int64_t)(0xffffffffu - (uint32_t)best) : -1);
}

// One digit of the radix selection.  s_hist holds the counts of the digit's REVERSED values among the keys still in the
// race; finds the reversed value at which the running count from the top reaches krem and how many keys of that digit
// value are still wanted.  Every lane returns both (sel[0], sel[1]).
__device__ __forceinline__ void sample_pick(const uint32_t* s_hist, uint32_t* s_wave, uint32_t* s_sel, uint32_t krem) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t c0 = s_hist[2 * tid], c1 = s_hist[2 * tid + 1], tot = c0 + c1;
    uint32_t incl = tot;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)incl, off);
        if (lane >= off) incl += o;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t ex = incl - tot;
    for (int w = 0; w < wave; ++w) ex += s_wave[w];
    if (ex < krem && krem <= ex + c0) {
        s_sel[0] = 2 * tid; s_sel[1] = krem - ex;
    } else if (ex + c0 < krem && krem <= ex + tot) {
        s_sel[0] = 2 * tid + 1; s_sel[1] = krem - ex - c0;
    }
    __syncthreads();
}

__global__ __launch_bounds__(SAMPLE_THREADS) void sample_topk_kernel(const SampleArgs a) {
    __shared__ uint32_t s_hist[SAMPLE_BINS];
    __shared__ uint64_t s_raw[AURA_SAMPLE_MAX_K];
    __shared__ uint64_t s_sorted[AURA_SAMPLE_MAX_K];
    __shared__ float s_e[AURA_SAMPLE_MAX_K];
    __shared__ float s_c[AURA_SAMPLE_MAX_K];
    __shared__ float s_tot[SAMPLE_NBLOCKS];
    __shared__ float s_base[SAMPLE_NBLOCKS];
    __shared__ uint32_t s_wave[2 * SAMPLE_WAVES];
    __shared__ uint32_t s_sel[2];
    __shared__ uint64_t s_red[SAMPLE_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = blockIdx.x;
    if (sample_row_finished(a, b)) return;
    const int V = a.V, k = a.k;
    const float* const zr = a.logits + b * a.row_stride;
    const uint8_t* const sr = a.seen ? a.seen + b * V : nullptr;
    uint32_t* const kr = a.keys + b * V;
    const uint32_t stream = a.streams ? (uint32_t)a.streams[b] : (uint32_t)b;

    // ---- pass 0: the keys, and the histogram of their top 11 bits
    for (int i = tid; i < SAMPLE_BINS; i += SAMPLE_THREADS) s_hist[i] = 0;
    __syncthreads();
    for (int i = tid; i < V; i += SAMPLE_THREADS) {
        const uint32_t key = sample_key(sample_value<true>(zr[i], sr && sr[i] != 0, a));
        kr[i] = key;
        atomicAdd(&s_hist[2047u - (key >> 21)], 1u);
    }
    __syncthreads();
    sample_pick(s_hist, s_wave, s_sel, (uint32_t)k);
    uint32_t T = (2047u - s_sel[0]) << 21, krem = s_sel[1];
    __syncthreads();

    // ---- pass 1: bits 20 .. 10 of the keys that share the top 11 bits
    for (int i = tid; i < SAMPLE_BINS; i += SAMPLE_THREADS) s_hist[i] = 0;
    __syncthreads();
    for (int i = tid; i < V; i += SAMPLE_THREADS) {
        const uint32_t key = kr[i];
        if ((key >> 21) == (T >> 21)) atomicAdd(&s_hist[2047u - ((key >> 10) & 2047u)], 1u);
    }
    __syncthreads();
    sample_pick(s_hist, s_wave, s_sel, krem);
    T |= (2047u - s_sel[0]) << 10; krem = s_sel[1];
    __syncthreads();

    // ---- pass 2: the low 10 bits (the upper half of the bins stays empty)
    for (int i = tid; i < SAMPLE_BINS; i += SAMPLE_THREADS) s_hist[i] = 0;
    __syncthreads();
    for (int i = tid; i < V; i += SAMPLE_THREADS) {
        const uint32_t key = kr[i];
        if ((key >> 10) == (T >> 10)) atomicAdd(&s_hist[1023u - (key & 1023u)], 1u);
    }
    __syncthreads();
    sample_pick(s_hist, s_wave, s_sel, krem);
    T |= 1023u - s_sel[0];
    const int need = (int)s_sel[1];                                     // of the keys equal to T, in id order
    const int above = k - need;                                         // = #(keys > T)

    // ---- compaction: wave w owns the ids [w per, (w + 1) per), per a multiple of 64
    const int per = ((V + SAMPLE_WAVES - 1) / SAMPLE_WAVES + 63) / 64 * 64;
    const int lo = wave * per, hi = min(V, lo + per);
    int n_gt = 0, n_eq = 0;
    for (int i0 = lo; i0 < hi; i0 += 64) {
        const uint32_t key = i0 + lane < hi ? kr[i0 + lane] : 0u;       // 0 is below every real key
        n_gt += __builtin_popcountll(sample_ballot(key > T));
        n_eq += __builtin_popcountll(sample_ballot(key == T));
    }
    if (lane == 0) { s_wave[wave] = (uint32_t)n_gt; s_wave[SAMPLE_WAVES + wave] = (uint32_t)n_eq; }
    __syncthreads();
    int gt_base = 0, eq_base = 0;
    for (int w = 0; w < wave; ++w) { gt_base += (int)s_wave[w]; eq_base += (int)s_wave[SAMPLE_WAVES + w]; }
    for (int i0 = lo; i0 < hi; i0 += 64) {
        const uint32_t key = i0 + lane < hi ? kr[i0 + lane] : 0u;
        const uint64_t bgt = sample_ballot(key > T), beq = sample_ballot(key == T);
        int pos = -1;
        if (key > T) pos = gt_base + sample_prefix(bgt);
        else if (key == T && eq_base + sample_prefix(beq) < need) pos = above + eq_base + sample_prefix(beq);
        if (pos >= 0 && pos < AURA_SAMPLE_MAX_K) s_raw[pos] = ((uint64_t)(~key) << 32) | (uint32_t)(i0 + lane);
        gt_base += __builtin_popcountll(bgt);
        eq_base += __builtin_popcountll(beq);
    }
    __syncthreads();

    // ---- order: (key descending, id ascending) = composite ascending
    if (tid < k) {
        const uint64_t mine = s_raw[tid];
        int rank = 0;
        for (int j = 0; j < k; ++j) rank += s_raw[j] < mine ? 1 : 0;
        s_sorted[rank] = mine;
    }
    __syncthreads();

    // ---- nucleus: lane j owns rank j
    const uint64_t comp = tid < k ? s_sorted[tid] : 0;
    const uint32_t id = (uint32_t)comp;
    const float z = sample_unkey(~(uint32_t)(comp >> 32));
    const float z0 = sample_unkey(~(uint32_t)(s_sorted[0] >> 32));
    const bool empty = !(z0 > -__builtin_inff());
    s_e[tid] = (tid < k && !empty) ? expf(z - z0) : 0.0f;
    __syncthreads();
    if (tid < SAMPLE_NBLOCKS) {
        float run = 0.0f;
#pragma unroll
        for (int q = 0; q < SAMPLE_BLOCK; ++q) {
            run = run + s_e[SAMPLE_BLOCK * tid + q];
            s_c[SAMPLE_BLOCK * tid + q] = run;
        }
        s_tot[tid] = run;
    }
    __syncthreads();
    if (tid == 0) {
        float base = 0.0f;
        for (int t = 0; t < SAMPLE_NBLOCKS; ++t) { s_base[t] = base; base = base + s_tot[t]; }
    }
    __syncthreads();
    const float c = s_base[tid / SAMPLE_BLOCK] + s_c[tid];
    __syncthreads();
    s_e[tid] = c;                                                       // s_e now holds the prefix sums
    __syncthreads();
    const float S = s_e[k - 1];
    const float thr = a.top_p * S;
    const bool kept = tid < k && !empty && (tid == 0 || a.top_p >= 1.0f || s_e[tid - 1] <= thr);

    // ---- draw
    const float d = kept ? sample_draw_key(z, id, stream, a) : -__builtin_inff();
    if (tid < k) {
        const int64_t o = b * k + tid;
        if (a.cand_ids) a.cand_ids[o] = (int32_t)id;
        if (a.cand_z) a.cand_z[o] = z;
        if (a.cand_cum) a.cand_cum[o] = c;
        if (a.cand_d) a.cand_d[o] = d;
    }
    const uint64_t bk = sample_ballot(kept);
    if (lane == 0) s_wave[wave] = (uint32_t)__builtin_popcountll(bk);
    const uint64_t best = sample_block_max((kept && z > -__builtin_inff()) ? sample_argmax_comp(d, id) : 0, s_red);
    if (tid == 0) {
        int n = 0;
        for (int w = 0; w < SAMPLE_WAVES; ++w) n += (int)s_wave[w];
        if (a.n_kept) a.n_kept[b] = n;
        sample_write_state(a, b, best ? (int64_t)(0xffffffffu - (uint32_t)best) : -1);
    }
}

inline bool sample_misaligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) != 0; }
inline bool sample_finite(float x) { return x == x && x - x == 0.0f; }

}  // namespace

extern "C" {

int64_t aura_sample_workspace_bytes(int64_t B, int64_t V, int64_t top_k, float temperature) {
    if (B < 1 || B > 0x7fffffffLL || V < 1 || V > AURA_SAMPLE_MAX_V || top_k < 0 || top_k > AURA_SAMPLE_MAX_K) return -1;
    if (!sample_finite(temperature) || temperature < 0.0f) return -1;
    if (top_k == 0 || temperature == 0.0f) return 0;
    return aura_align256(B * V * 4);
}

int aura_sample_next(const float* logits, int64_t row_stride, int64_t B, int64_t V, uint8_t* seen_or_null,
                     uint8_t* finished_or_null, const int64_t* stream_ids_or_null, float penalty, int penalty_rule,
                     float temperature, int64_t top_k, float top_p, uint64_t seed, uint64_t step, int64_t eos_id,
                     int64_t pad_id, int64_t* tokens, int64_t token_stride, int32_t* cand_ids, float* cand_z,
                     float* cand_cum, float* cand_d, int32_t* n_kept, void* workspace, int64_t workspace_bytes,
                     void* stream) {
    if (B < 1 || B > 0x7fffffffLL || V < 1 || V > AURA_SAMPLE_MAX_V) return AURA_E_INVAL;
    if (top_k < 0 || top_k > AURA_SAMPLE_MAX_K) return AURA_E_INVAL;
    if (!sample_finite(temperature) || temperature < 0.0f) return AURA_E_INVAL;
    if (!sample_finite(penalty) || penalty <= 0.0f) return AURA_E_INVAL;
    if (!(top_p >= 0.0f)) return AURA_E_INVAL;                                  // (NaN fails)
    if (top_k == 0 && top_p < 1.0f) return AURA_E_INVAL;
    if (penalty_rule != AURA_PENALTY_DIVIDE && penalty_rule != AURA_PENALTY_SIGNED) return AURA_E_INVAL;
    if (!logits || !tokens || row_stride < V || token_stride < 1) return AURA_E_INVAL;
    if (sample_misaligned(tokens, 8) || sample_misaligned(stream_ids_or_null, 8) || sample_misaligned(logits, 4) ||
        sample_misaligned(cand_ids, 4) || sample_misaligned(cand_z, 4) || sample_misaligned(cand_cum, 4) ||
        sample_misaligned(cand_d, 4) || sample_misaligned(n_kept, 4))
        return AURA_E_ALIGN;
    const int64_t need = aura_sample_workspace_bytes(B, V, top_k, temperature);
    if (need > 0) {
        if (!workspace || workspace_bytes < need) return AURA_E_INVAL;
        if (sample_misaligned(workspace, 256)) return AURA_E_ALIGN;
    }
    SampleArgs a;
    a.logits = logits; a.row_stride = row_stride; a.seen = seen_or_null; a.finished = finished_or_null;
    a.streams = stream_ids_or_null; a.tokens = tokens; a.token_stride = token_stride;
    a.cand_ids = cand_ids; a.cand_z = cand_z; a.cand_cum = cand_cum; a.cand_d = cand_d; a.n_kept = n_kept;
    a.keys = static_cast<uint32_t*>(workspace);
    a.V = (int)V; a.k = (int)(top_k < V ? top_k : V);
    a.rule = penalty_rule; a.penalty = penalty; a.temperature = temperature; a.top_p = top_p;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
    a.step_lo = (uint32_t)step; a.step_hi = (uint32_t)(step >> 32);
    a.eos_id = eos_id; a.pad_id = pad_id;
    const dim3 grid((unsigned)B), block(SAMPLE_THREADS);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (temperature == 0.0f) {
        a.cand_ids = nullptr; a.cand_z = a.cand_cum = a.cand_d = nullptr; a.n_kept = nullptr;
        hipLaunchKernelGGL(sample_argmax_kernel<true>, grid, block, 0, s, a);
    } else if (top_k == 0) {
        hipLaunchKernelGGL(sample_argmax_kernel<false>, grid, block, 0, s, a);
    } else {
        hipLaunchKernelGGL(sample_topk_kernel, grid, block, 0, s, a);
    }
    return aura_check_launch();
}

}  // extern "C"
