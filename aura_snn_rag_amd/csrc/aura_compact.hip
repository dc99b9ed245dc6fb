// aura_compact.hip -- in-place compaction of the episodic bank (aura_bank_compact), for gfx950: rows src[0 .. n) of the
// six row arrays (features, locations, metadata, inv_norm and -- when given -- the row-ordered bf16 shadow and rho)
// move to rows dst0 .. dst0 + n - 1, as if every source were read before any destination is written.
// [build-side] no upstream counterpart (the reference's pruning ends in `pass`).
//
// src ascends strictly and dst0 + i <= src[i], so destinations never lie above their sources and both ascend.  The
// rows are taken in rounds of CP_ROUND = 4096 in ascending order; a round is
//   direct  when its whole destination range lies below its first source (dst0 + b - 1 < src[a] for the round
//           [a, b)): every source of the round lies above every destination of the round, so each row is read and
//           written once, straight from its old place to its new one;
//   staged  otherwise: the round's rows are gathered into one half of the workspace and stored from there by the NEXT
//           launch.
// Launch k stores round k - 1 (if it was staged) and gathers or moves round k, so a call is rounds + 1 launches.  The
// two parts of a launch never touch the same memory: the store writes rows < dst0 + a_k <= src[a_k] and reads the
// workspace half of round k - 1 only; round k reads rows >= src[a_k] and writes the other half (staged) or rows
// dst0 + [a_k, b_k) (direct).  Whether a round is direct is decided on the device from src[a] (every workgroup reads
// that one entry): the host never sees src, so nothing is synchronised.  A row with dst0 + i == src[i] is skipped
// by both parts (such rows form a prefix of src).
// One wave moves one row: 16-byte accesses, consecutive lanes on consecutive chunks, up to four loads in flight per
// lane before the first store; a scalar path takes feature rows that are not made of aligned 16-byte chunks.  A
// source or destination outside [0, rows), or a source below its destination, is skipped before it becomes an address.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/aura_hip.h"
#include "aura_common.inl"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int CP_ROUND = 4096;           // rows per round (and per workspace half)

struct RowArrays {
    float* bank;          // [.][D]
    float* loc;           // [.][S]
    float* meta;          // [.][4]
    float* inv;           // [.]
    uint16_t* shadow;     // [.][D] or null
    float* rho;           // [.] or null
};

inline RowArrays carve_half(char* p, int64_t& o, int64_t D, int64_t S, bool has_shadow) {
    RowArrays w;
    auto take = [&](int64_t b) { char* r = p ? p + o : nullptr; o += aura_align256(b); return r; };
    w.bank = reinterpret_cast<float*>(take(4LL * CP_ROUND * D));
    w.loc = reinterpret_cast<float*>(take(4LL * CP_ROUND * (S > 0 ? S : 1)));
    w.meta = reinterpret_cast<float*>(take(16LL * CP_ROUND));
    w.inv = reinterpret_cast<float*>(take(4LL * CP_ROUND));
    w.shadow = has_shadow ? reinterpret_cast<uint16_t*>(take(2LL * CP_ROUND * D)) : nullptr;
    w.rho = has_shadow ? reinterpret_cast<float*>(take(4LL * CP_ROUND)) : nullptr;
    return w;
}

// nchunks consecutive elements of type V, one wave: four loads in flight per lane, then the stores
template <typename V>
__device__ __forceinline__ void cp_copy(const V* __restrict__ s, V* __restrict__ d, int nchunks, int lane) {
    for (int c0 = 0; c0 < nchunks; c0 += 256) {
        V v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + 64 * j + lane;
            if (c < nchunks) v[j] = s[c];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + 64 * j + lane;
            if (c < nchunks) d[c] = v[j];
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void cp_move_row(const RowArrays& from, int64_t fr, const RowArrays& to, int64_t tr, int D,
                                            int S, int lane) {
    if (VEC)
        cp_copy(reinterpret_cast<const u32x4*>(from.bank + fr * D), reinterpret_cast<u32x4*>(to.bank + tr * D), D / 4, lane);
    else
        cp_copy(from.bank + fr * D, to.bank + tr * D, D, lane);
    if (from.shadow)                                                  // D % 8 == 0: rows of whole 16-byte chunks
        cp_copy(reinterpret_cast<const u32x4*>(from.shadow + fr * D), reinterpret_cast<u32x4*>(to.shadow + tr * D), D / 8,
                lane);
    cp_copy(from.loc + fr * S, to.loc + tr * S, S, lane);
    if (lane < 4) to.meta[tr * 4 + lane] = from.meta[fr * 4 + lane];
    if (lane == 4) to.inv[tr] = from.inv[fr];
    if (lane == 5 && from.rho) to.rho[tr] = from.rho[fr];
}

// One launch: workgroups [0, sblocks) store the staged round [sa, sa + sn) from ws_store; the others take the round
// [ga, ga + gn): straight to its destination when it is direct, into ws_gather otherwise.  One wave per row.
template <bool VEC>
__global__ __launch_bounds__(256) void cp_round_kernel(RowArrays g, RowArrays ws_store, RowArrays ws_gather, int64_t rows,
                                                       int D, int S, const int32_t* __restrict__ src, int64_t dst0,
                                                       int64_t sa, int sn, int sblocks, int64_t ga, int gn) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool store = (int)blockIdx.x < sblocks;
    const int64_t a = store ? sa : ga;
    const int cnt = store ? sn : gn;
    const int local = ((int)blockIdx.x - (store ? 0 : sblocks)) * 4 + wave;
    if (local >= cnt) return;
    const bool direct = dst0 + a + cnt - 1 < (int64_t)src[a];
    if (store && direct) return;                                      // the round went straight to its place
    const int64_t i = a + local;
    const int64_t s = src[i], d = dst0 + i;
    if (s <= d || s >= rows || d < 0) return;                         // in place already, or not a row of the arrays
    if (store)
        cp_move_row<VEC>(ws_store, local, g, d, D, S, lane);
    else if (direct)
        cp_move_row<VEC>(g, s, g, d, D, S, lane);
    else
        cp_move_row<VEC>(g, s, ws_gather, local, D, S, lane);
}

}  // namespace

extern "C" {

int64_t aura_bank_compact_round_rows(void) { return CP_ROUND; }

int64_t aura_bank_compact_workspace_bytes(int64_t D, int64_t S, int has_shadow) {
    if (D < 1 || D > 4096 || S < 0 || S > 4096) return -1;
    if (has_shadow && D % 8 != 0) return -1;
    int64_t o = 0;
    carve_half(nullptr, o, D, S, has_shadow != 0);
    carve_half(nullptr, o, D, S, has_shadow != 0);
    return o;
}

int aura_bank_compact(float* bank, float* loc, float* meta, float* inv_norm, uint16_t* shadow_bf16, float* rho,
                      int64_t rows, int64_t D, int64_t S, const int32_t* src, int64_t n, int64_t dst0, void* workspace,
                      int64_t workspace_bytes, void* stream) {
    const bool has_shadow = shadow_bf16 != nullptr;
    if (has_shadow != (rho != nullptr)) return AURA_E_INVAL;
    const int64_t need = aura_bank_compact_workspace_bytes(D, S, has_shadow ? 1 : 0);
    if (need < 0 || rows < 0 || rows > 0x7fffffffLL || n < 0 || dst0 < 0 || dst0 > rows || n > rows - dst0)
        return AURA_E_INVAL;
    if (n == 0) return AURA_OK;
    if (!bank || !meta || !inv_norm || !src || (S > 0 && !loc) || !workspace || workspace_bytes < need) return AURA_E_INVAL;
    if (reinterpret_cast<uintptr_t>(workspace) & 255) return AURA_E_ALIGN;
    if (has_shadow && (reinterpret_cast<uintptr_t>(shadow_bf16) & 15)) return AURA_E_ALIGN;
    if ((reinterpret_cast<uintptr_t>(bank) | reinterpret_cast<uintptr_t>(loc) | reinterpret_cast<uintptr_t>(meta) |
         reinterpret_cast<uintptr_t>(inv_norm) | reinterpret_cast<uintptr_t>(rho) | reinterpret_cast<uintptr_t>(src)) & 3)
        return AURA_E_ALIGN;
    const bool vec = D % 4 == 0 && !(reinterpret_cast<uintptr_t>(bank) & 15);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const RowArrays g = {bank, loc, meta, inv_norm, shadow_bf16, rho};
    int64_t o = 0;
    RowArrays half[2];
    half[0] = carve_half(static_cast<char*>(workspace), o, D, S, has_shadow);
    half[1] = carve_half(static_cast<char*>(workspace), o, D, S, has_shadow);
    const int64_t rounds = (n + CP_ROUND - 1) / CP_ROUND;
    for (int64_t k = 0; k <= rounds; ++k) {
        // store round k - 1, take round k
        const int64_t sa = k > 0 ? (k - 1) * CP_ROUND : 0;
        const int sn = k > 0 ? (int)(n - sa < CP_ROUND ? n - sa : CP_ROUND) : 0;
        const int64_t ga = k < rounds ? k * CP_ROUND : 0;
        const int gn = k < rounds ? (int)(n - ga < CP_ROUND ? n - ga : CP_ROUND) : 0;
        const int sblocks = (sn + 3) / 4, gblocks = (gn + 3) / 4;
        const RowArrays& wst = half[(k + 1) & 1];
        const RowArrays& wga = half[k & 1];
        if (vec)
            hipLaunchKernelGGL(cp_round_kernel<true>, dim3((unsigned)(sblocks + gblocks)), dim3(256), 0, st, g, wst, wga,
                               rows, (int)D, (int)S, src, dst0, sa, sn, sblocks, ga, gn);
        else
            hipLaunchKernelGGL(cp_round_kernel<false>, dim3((unsigned)(sblocks + gblocks)), dim3(256), 0, st, g, wst, wga,
                               rows, (int)D, (int)S, src, dst0, sa, sn, sblocks, ga, gn);
        const int rc = aura_check_launch();
        if (rc != AURA_OK) return rc;
    }
    return AURA_OK;
}

}  // extern "C"
