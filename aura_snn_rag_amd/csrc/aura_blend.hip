// aura_blend.hip -- blending merges: a repeated memory moves toward the rows that repeat it (gfx950).
// The rule is stated once, in include/aura_hip.h ("Blending merges"); the comments here are about how it is computed.
//   grouping   on the device, from the two int32 arrays aura_bank_find_repeats left there.  One wave per batch row: it
//              reads the row's group key, then ballots over the arrays in chunks of 64 rows.  A wave whose row is not
//              the FIRST member of its group retires (so does the wave of a kept row, or of an entry out of range):
//              every group is walked by exactly one wave, its members in ascending order.
//   chain      the running row g lives in LDS, D floats per wave (16 KB at D = 4096, four waves per workgroup), the
//              feature dimension across the lanes, 16-byte accesses when D % 4 == 0.  A lane only ever touches its own
//              columns of g until the chain ends, so the walk needs no barrier.  g = g + beta * (f - g) is a
//              subtraction, a product and a sum: contraction is off (aura_common.inl's pragma, the Makefile's flag).
//   derived    the final row goes to its place and, for a row of the bank, 1/||g|| (wave_row_sumsq), the bf16 shadow
//              row with its rho and the row's entry of the list-sorted image (shadow_convert_row) follow in the same
//              launch from the LDS copy: the arithmetic of aura_bank_row_norms / aura_bank_shadow_update by
//              construction (aura_row.inl).
// A key row is written by its one wave and read by nobody else; member rows are read and never written: a valid input
// has no race, and an invalid one (a leader that is not a kept row) is refused by blend_key before it becomes a key.
// HBM traffic: 4 D bytes per member, 8 D per key (+ 2 D per bf16 image kept): a few hundred KB per call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/aura_hip.h"
#include "aura_common.inl"

namespace {

#include "aura_row.inl"

constexpr int BLEND_NONE = -1;          // the row is kept, or its entry is out of range: a member of nothing

struct BlendArgs {
    float* bank;                        // [rows][D]
    float* inv_norm;                    // [rows]
    int64_t N, rows, D;
    const float* feats;                 // batch row i = feats + i * D (a slab: bank + feats_row0 * D)
    float* out;                         // where a blended batch key goes: out + j * D (a slab: the same rows)
    int64_t out_row0;                   // bank row of batch row 0 (a slab), -1 when `out` is not the bank
    int64_t n;
    const int32_t* stored;
    const int32_t* leader;
    float beta;
    uint16_t* shadow;                   // row-ordered bf16 shadow or NULL
    float* rho;
    int64_t shadow_upto;
    uint16_t* sorted_bf16;              // list-sorted image or NULL
    const int32_t* sorted_rows;
    const int32_t* pos_of_row;
    int64_t n_sorted;
    bool image_f16;                     // the list-sorted image is IEEE half (AURA_IMAGE_F16)
    float* rho16;                       // ... and this, when given, receives its residual norm; rho the bf16 one as ever
};

// Group key of batch row i as one int: held row r -> r; batch row j -> -2 - j; BLEND_NONE otherwise.  Every id is
// checked here, before it becomes an address: a stored target outside [0, N), a leader outside [0, i) or one that is
// not itself a kept row make the row a member of nothing.
__device__ __forceinline__ int blend_key(const BlendArgs& a, int i) {
    const int st = a.stored[i];
    if (st >= 0) return st < a.N ? st : BLEND_NONE;
    const int ld = a.leader[i];
    if (ld < 0 || ld >= i) return BLEND_NONE;
    if (a.stored[ld] >= 0 || a.leader[ld] >= 0) return BLEND_NONE;
    return -2 - ld;
}

template <bool VEC4>
__global__ __launch_bounds__(256) void bank_blend_kernel(const BlendArgs a) {
    extern __shared__ __attribute__((aligned(16))) float s_g[];      // [4][D]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i64 = (int64_t)blockIdx.x * 4 + wave;
    if (i64 >= a.n) return;
    const int i = (int)i64, n = (int)a.n;
    const int64_t D = a.D;
    const int key = blend_key(a, i);                // the same on every lane
    if (key == BLEND_NONE) return;
    float* const g = s_g + (int64_t)wave * D;
    const float beta = a.beta;
    bool started = false;
    for (int base = 0; base < n; base += 64) {
        const int m = base + lane;
        const unsigned long long members = __ballot(m < n && blend_key(a, m) == key);
        unsigned long long todo = members;
        if (!started) {
            if (base + 64 <= i) {                   // a chunk before this row's: any member there is an earlier one
                if (members) return;
                continue;
            }
            if (members & ((1ull << (i - base)) - 1ull)) return;
            started = true;
            const float* const k0 = key >= 0 ? a.bank + (int64_t)key * D : a.feats + (int64_t)(-2 - key) * D;
            if (VEC4) {
                for (int64_t c = lane * 4; c < D; c += 256)
                    *reinterpret_cast<float4*>(g + c) = *reinterpret_cast<const float4*>(k0 + c);
            } else {
                for (int64_t c = lane; c < D; c += 64) g[c] = k0[c];
            }
        }
        while (todo) {                              // members in ascending order
            const int b = __ffsll(todo) - 1;
            todo &= todo - 1ull;
            const float* const f = a.feats + (int64_t)(base + b) * D;
            if (VEC4) {
                for (int64_t c = lane * 4; c < D; c += 256) {
                    float4 gv = *reinterpret_cast<const float4*>(g + c);
                    const float4 fv = *reinterpret_cast<const float4*>(f + c);
                    gv.x = gv.x + beta * (fv.x - gv.x);
                    gv.y = gv.y + beta * (fv.y - gv.y);
                    gv.z = gv.z + beta * (fv.z - gv.z);
                    gv.w = gv.w + beta * (fv.w - gv.w);
                    *reinterpret_cast<float4*>(g + c) = gv;
                }
            } else {
                for (int64_t c = lane; c < D; c += 64) {
                    const float gv = g[c];
                    g[c] = gv + beta * (f[c] - gv);
                }
            }
        }
    }
    // the final row to its place: the held target, the slab's own row, or the caller's copy of the batch
    const int64_t kr = key >= 0 ? (int64_t)key : (a.out_row0 >= 0 ? a.out_row0 + (-2 - key) : -1);
    float* const dst = key >= 0 ? a.bank + (int64_t)key * D : a.out + (int64_t)(-2 - key) * D;
    if (VEC4) {
        for (int64_t c = lane * 4; c < D; c += 256)
            *reinterpret_cast<float4*>(dst + c) = *reinterpret_cast<const float4*>(g + c);
    } else {
        for (int64_t c = lane; c < D; c += 64) dst[c] = g[c];
    }
    if (kr < 0) return;                             // (the write kernels derive the rest when they store the row)
    // the conversions below read g across lanes: the wave's own LDS writes first
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const float s = wave_row_sumsq(g, D, lane, VEC4);
    const float inv = 1.0f / fmaxf(sqrtf(s), 1e-12f);
    if (lane == 0) a.inv_norm[kr] = inv;
    if (a.shadow && kr < a.shadow_upto) {
        const float r = shadow_convert_row(g, inv, a.shadow + kr * D, D, lane);
        if (lane == 0) a.rho[kr] = r;
    }
    if (a.sorted_bf16) {
        const int p = a.pos_of_row[kr];
        if (p >= 0 && p < a.n_sorted && a.sorted_rows[p] == (int32_t)kr) {
            float r, r16 = 0.0f;
            if (a.image_f16) r16 = shadow_convert_row_f16(g, inv, a.sorted_bf16 + (int64_t)p * D, D, lane, r);
            else r = shadow_convert_row(g, inv, a.sorted_bf16 + (int64_t)p * D, D, lane);
            if (lane == 0) {
                a.rho[kr] = r;
                if (a.image_f16 && a.rho16) a.rho16[kr] = r16;
            }
        }
    }
}

inline bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace

extern "C" {

// rho16 (optional, AURA_IMAGE_F16 only) follows the half image, rho the bf16 residual
int aura_bank_blend(float* bank, float* inv_norm, int64_t N, int64_t rows, int64_t D, const float* feats,
                    int64_t feats_row0, int64_t n, const int32_t* stored_target, const int32_t* batch_leader,
                    float beta, float* out_feats, uint16_t* shadow_bf16, float* rho, int64_t shadow_upto,
                    uint16_t* sorted_bf16, float* rho16, const int32_t* sorted_rows, const int32_t* pos_of_row,
                    int64_t n_sorted, int image_format, void* stream) {
    if (image_format != AURA_IMAGE_F16 && (image_format != AURA_IMAGE_BF16 || rho16)) return AURA_E_INVAL;
    const bool image_f16 = image_format == AURA_IMAGE_F16;
    if (n < 0 || n > 1024 || D < 1 || D > 4096 || N < 0 || rows < N || rows > 0x7fffffff) return AURA_E_INVAL;
    if (!(beta > 0.0f && beta <= 1.0f)) return AURA_E_INVAL;
    if (feats_row0 < -1) return AURA_E_INVAL;
    if (feats_row0 >= 0 && (feats_row0 < N || feats_row0 + n > rows)) return AURA_E_INVAL;
    const bool has_image = sorted_bf16 != nullptr;
    if ((sorted_rows != nullptr) != has_image || (pos_of_row != nullptr) != has_image) return AURA_E_INVAL;
    if ((rho != nullptr) != (shadow_bf16 != nullptr || has_image)) return AURA_E_INVAL;
    if (shadow_bf16 && (shadow_upto < 0 || shadow_upto > rows)) return AURA_E_INVAL;
    if (has_image && n_sorted < 0) return AURA_E_INVAL;
    if ((shadow_bf16 || has_image) && (D & 7)) return AURA_E_INVAL;
    if (n == 0) return AURA_OK;
    if (!bank || !inv_norm || !stored_target || !batch_leader) return AURA_E_INVAL;
    if (feats_row0 < 0 && (!feats || !out_feats)) return AURA_E_INVAL;
    if (misaligned16(shadow_bf16) || misaligned16(sorted_bf16)) return AURA_E_ALIGN;
    BlendArgs a;
    a.bank = bank; a.inv_norm = inv_norm; a.N = N; a.rows = rows; a.D = D;
    a.feats = feats_row0 >= 0 ? bank + feats_row0 * D : feats;
    a.out = feats_row0 >= 0 ? bank + feats_row0 * D : out_feats;
    a.out_row0 = feats_row0;
    a.n = n; a.stored = stored_target; a.leader = batch_leader; a.beta = beta;
    a.shadow = shadow_bf16; a.rho = rho; a.shadow_upto = shadow_bf16 ? shadow_upto : 0;
    a.sorted_bf16 = sorted_bf16; a.sorted_rows = sorted_rows; a.pos_of_row = pos_of_row; a.n_sorted = n_sorted;
    a.image_f16 = image_f16 && has_image; a.rho16 = a.image_f16 ? rho16 : nullptr;
    // 16-byte accesses exactly where aura_bank_row_norms takes them (D % 4 == 0, an aligned bank): the sum of squares
    // must associate alike.  Batch rows that such a bank cannot be read with are refused, not read narrower.
    const bool vec4 = (D % 4 == 0) && !misaligned16(bank);
    if (vec4 && (misaligned16(a.feats) || misaligned16(a.out))) return AURA_E_ALIGN;
    if ((shadow_bf16 || has_image) && !vec4) return AURA_E_ALIGN;
    const dim3 grid((unsigned)((n + 3) / 4)), block(256);
    const size_t lds = (size_t)4 * D * sizeof(float);             // <= 64 KB
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec4) hipLaunchKernelGGL(bank_blend_kernel<true>, grid, block, lds, s, a);
    else hipLaunchKernelGGL(bank_blend_kernel<false>, grid, block, lds, s, a);
    return aura_check_launch();
}

}  // extern "C"
