// aura_stdp.hip -- timestep STDP: traces and weight update in one fused launch plus a small reduction (gfx950).
// The rule is stated once, in include/aura_hip.h ("STDP"); the comments here are about how it is computed.
//   tiles      a workgroup (256 threads) owns 128 outputs x 128 inputs of dW and the batch rows [b_lo, b_hi) of its
//              split (blockIdx.z).  It walks those rows' steps as one flat sequence s = (b - b_lo) T + t, 16 steps
//              (a chunk) at a time, so short T wastes no matrix work except in the split's last chunk.
//   staging    the tile has 128 post columns and 128 pre columns: one thread each.  A thread keeps its column's trace in
//              a register from step to step (x or y never reach HBM, except the final value of every row), loads the
//              16 values of the next chunk, and, after the MFMAs of the current chunk, turns them into the two k-slots
//              of every step:   slot 0 = (a_plus post_t , x_t)      -- x_t includes step t
//                               slot 1 = (-a_minus y_t-, pre_t)     -- y_t- = fl(lambda_post y_t-1): the post trace
//                                                                      at t before the step's own spike
//              A step beyond the split's last one is staged as zeros on both sides.
//   LDS        image[buffer 2][side 2][group of 4 steps 4][slot 2][column 128] float4 = 64 KB: a thread writes the four
//              steps of a group with one 16-byte store, a lane reads one float4 per 32 x 32 operand -- consecutive lanes
//              16 bytes apart both ways, so neither access has a bank conflict.  Two buffers, one barrier per chunk.
//   MFMA       v_mfma_f32_32x32x2_f32 through aura_mfma_f32_x4: exact fp32, bitwise a k-ordered fmaf chain.  A wave owns
//              64 x 64 of the tile (2 x 2 accumulators of 32 x 32): 64 MFMAs per chunk against 16 loads, ~50 VALU
//              instructions and 8 LDS stores of staging.
//   partials   every workgroup stores its tile of its split's sum to the workspace [split][O][I]; stdp_finish_kernel
//              adds the splits in ascending order, divides by B and writes dW and/or the clamped weights.
// The summation order is a function of (B, T, I, O) alone: no atomics, no dependence on the device.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/aura_hip.h"
#include "aura_common.inl"

namespace {

constexpr int STDP_TILE = 128;          // outputs and inputs per workgroup
constexpr int STDP_CHUNK = 16;          // steps staged per barrier
constexpr int STDP_GROUPS = STDP_CHUNK / 4;
// Workgroups aimed at: two rounds of two per CU on a 256-CU part, so that the last round is nearly full whatever the
// tile count (144 tiles x 7 splits = 1008 of 1024); a constant, never queried from the device
constexpr int64_t STDP_TARGET_WGS = 1024;
constexpr int64_t STDP_MAX_SPLIT = 64;

inline int64_t stdp_tiles(int64_t n) { return (n + STDP_TILE - 1) / STDP_TILE; }

// How many ways the batch rows are split: enough workgroups to fill the chip when the O x I grid alone does not,
// from the shapes only.
inline int64_t stdp_splits(int64_t B, int64_t I, int64_t O) {
    int64_t s = STDP_TARGET_WGS / (stdp_tiles(I) * stdp_tiles(O));
    if (s > STDP_MAX_SPLIT) s = STDP_MAX_SPLIT;
    if (s > B) s = B;
    return s < 1 ? 1 : s;
}

struct StdpArgs {
    const void* pre;                    // [B][T][I], or [B][I] when time-invariant
    const void* post;                   // [B][T][O]
    const float* x_in;                  // [B][I] or NULL (zero)
    const float* y_in;                  // [B][O] or NULL (zero)
    float* x_out;                       // [B][I] or NULL (not wanted)
    float* y_out;                       // [B][O] or NULL
    float* part;                        // [splits][O][I]
    float lambda_pre, lambda_post, a_plus, neg_a_minus;
    int64_t B, T, I, O;
    int splits, pre_invariant;
};

template <bool BF16>
__device__ __forceinline__ float stdp_load(const void* p, int64_t idx) {
    if (BF16) return __uint_as_float((uint32_t)static_cast<const uint16_t*>(p)[idx] << 16);
    return static_cast<const float*>(p)[idx];
}

// INV: pre is [B][I], the same at every step: the pre side's element index moves on once per row, not per step.
template <bool BF16, bool INV>
__global__ __launch_bounds__(256, 2) void stdp_partial_kernel(const StdpArgs a) {
    __shared__ float4 s_img[2][2][STDP_GROUPS][2][STDP_TILE];           // 64 KB
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t T = a.T;
    const int split = blockIdx.z;
    const int64_t b_lo = a.B * split / a.splits, b_hi = a.B * (split + 1) / a.splits;
    const int64_t S = (b_hi - b_lo) * T;                                 // flat steps of this split
    const int64_t nchunks = (S + STDP_CHUNK - 1) / STDP_CHUNK;

    // ---- the staging role of this thread: waves 0, 1 the post columns (side 0), waves 2, 3 the pre columns (side 1)
    const bool is_post = wave < 2;
    const int col = tid & (STDP_TILE - 1);
    const int64_t N = is_post ? a.O : a.I;                               // row length of this side
    const int64_t n0 = (int64_t)(is_post ? blockIdx.y : blockIdx.x) * STDP_TILE;
    const bool col_ok = n0 + col < N;
    const void* const src = is_post ? a.post : a.pre;
    const float* const tr_in = is_post ? a.y_in : a.x_in;
    // final traces are written once: by tile row 0 for x, by tile column 0 for y
    float* const tr_out = is_post ? (blockIdx.x == 0 ? a.y_out : nullptr) : (blockIdx.y == 0 ? a.x_out : nullptr);
    const float lam = is_post ? a.lambda_post : a.lambda_pre;
    const float ap = a.a_plus, nam = a.neg_a_minus;

    float v[STDP_CHUNK];                                                 // the chunk in flight
    // where the loads are: flat step, step within the row (INV only), element index of this column at that step
    int64_t ld_s = 0, ld_idx = ((INV && !is_post) ? b_lo : b_lo * T) * N + n0 + col;
    int ld_t = 0;
    // where the recursion is: flat step, step within the row, element index of this column's trace of that row
    int64_t st_s = 0, tr_idx = b_lo * N + n0 + col;
    int st_t = 0;
    const int t_last = (int)T - 1;
    float tr = 0.0f;

    auto load_chunk = [&]() {
#pragma unroll
        for (int j = 0; j < STDP_CHUNK; ++j) {
            // every load is issued (element 0 stands in for one that is not wanted): a branch around a load would
            // make the compiler wait for each before the next.  The value is first looked at when it is staged.
            v[j] = stdp_load<BF16>(src, (col_ok && ld_s < S) ? ld_idx : 0);
            ++ld_s;
            if (INV) {
                const bool wrap = ld_t == t_last;
                ld_t = wrap ? 0 : ld_t + 1;
                if (is_post || wrap) ld_idx += N;
            } else {
                ld_idx += N;
            }
        }
    };
    auto stage_chunk = [&](int buf) {
#pragma unroll
        for (int g = 0; g < STDP_GROUPS; ++g) {
            float s0[4], s1[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool live = st_s < S;                              // uniform over the workgroup
                if (live && st_t == 0) tr = (tr_in && col_ok) ? tr_in[tr_idx] : 0.0f;
                const float x = (live && col_ok) ? v[g * 4 + j] : 0.0f;
                const float decayed = lam * tr;                          // two roundings: contraction is off
                tr = decayed + x;
                const float f0 = is_post ? ap * x : tr;
                const float f1 = is_post ? nam * decayed : x;
                s0[j] = live ? f0 : 0.0f;
                s1[j] = live ? f1 : 0.0f;
                const bool wrap = st_t == t_last;
                if (live && wrap && tr_out && col_ok) tr_out[tr_idx] = tr;
                ++st_s;
                st_t = wrap ? 0 : st_t + 1;
                if (wrap) tr_idx += N;
            }
            s_img[buf][is_post ? 0 : 1][g][0][col] = make_float4(s0[0], s0[1], s0[2], s0[3]);
            s_img[buf][is_post ? 0 : 1][g][1][col] = make_float4(s1[0], s1[1], s1[2], s1[3]);
        }
    };

    // ---- the MFMA role: wave (wr, wc) owns outputs [64 wr, +64) x inputs [64 wc, +64) of the tile
    const int wr = wave >> 1, wc = wave & 1, half = lane >> 5, l31 = lane & 31;
    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.0f;

    load_chunk();
    stage_chunk(0);
    __syncthreads();
    for (int64_t c = 0; c < nchunks; ++c) {
        const int buf = (int)(c & 1);
        const bool more = c + 1 < nchunks;
        if (more) load_chunk();
#pragma unroll
        for (int g = 0; g < STDP_GROUPS; ++g) {
            const float4 a0 = s_img[buf][0][g][half][wr * 64 + l31];
            const float4 a1 = s_img[buf][0][g][half][wr * 64 + 32 + l31];
            const float4 b0 = s_img[buf][1][g][half][wc * 64 + l31];
            const float4 b1 = s_img[buf][1][g][half][wc * 64 + 32 + l31];
            acc[0][0] = aura_mfma_f32_x4(a0, b0, acc[0][0]);
            acc[0][1] = aura_mfma_f32_x4(a0, b1, acc[0][1]);
            acc[1][0] = aura_mfma_f32_x4(a1, b0, acc[1][0]);
            acc[1][1] = aura_mfma_f32_x4(a1, b1, acc[1][1]);
        }
        if (more) stage_chunk(buf ^ 1);
        __syncthreads();
    }

    // ---- this split's tile to the workspace: accumulator register r of lane l is row (r&3) + 8 (r>>2) + 4 (l>>5),
    // column l & 31 of its 32 x 32 block
    float* const part = a.part + (int64_t)split * a.O * a.I;
    const int64_t o0 = (int64_t)blockIdx.y * STDP_TILE + wr * 64, i0 = (int64_t)blockIdx.x * STDP_TILE + wc * 64;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int64_t i = i0 + n * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t o = o0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (o < a.O && i < a.I) part[o * a.I + i] = acc[m][n][r];
            }
        }
}

// dW = (sum of the splits, ascending) / B;  W' = clamp(W + lr dW).  One thread per four inputs.
__global__ __launch_bounds__(256) void stdp_finish_kernel(const float* __restrict__ part, int splits, int64_t n4,
                                                          float fB, float* W, float* dw_out, float lr, float w_min,
                                                          float w_max) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n4) return;
    const float4* const p = reinterpret_cast<const float4*>(part);
    float4 s = p[k];
    for (int z = 1; z < splits; ++z) {
        const float4 q = p[(int64_t)z * n4 + k];
        s.x = s.x + q.x; s.y = s.y + q.y; s.z = s.z + q.z; s.w = s.w + q.w;
    }
    s.x = s.x / fB; s.y = s.y / fB; s.z = s.z / fB; s.w = s.w / fB;
    if (dw_out) reinterpret_cast<float4*>(dw_out)[k] = s;
    if (W) {
        float4 w = reinterpret_cast<float4*>(W)[k];
        w.x = fminf(fmaxf(w.x + lr * s.x, w_min), w_max);
        w.y = fminf(fmaxf(w.y + lr * s.y, w_min), w_max);
        w.z = fminf(fmaxf(w.z + lr * s.z, w_min), w_max);
        w.w = fminf(fmaxf(w.w + lr * s.w, w_min), w_max);
        reinterpret_cast<float4*>(W)[k] = w;
    }
}

inline bool stdp_shape_ok(int64_t B, int64_t T, int64_t I, int64_t O) {
    if (B < 1 || T < 1 || I < 1 || O < 1) return false;
    if (B > 0x7fffffff || T > 0x7fffffff || I > 0x7fffffff || O > 0x7fffffff) return false;
    if (stdp_tiles(O) > 65535) return false;
    // every flat index stays far below 2^63
    const double big = (double)B * (double)T * (double)(I > O ? I : O);
    return big < 4.0e18 && (double)O * (double)I <= 1099511627776.0;       // 2^40: the finish grid stays below 2^31
}

inline bool misaligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) != 0; }

}  // namespace

extern "C" {

int64_t aura_stdp_workspace_bytes(int64_t B, int64_t T, int64_t I, int64_t O) {
    if (!stdp_shape_ok(B, T, I, O)) return -1;
    return aura_align256(stdp_splits(B, I, O) * O * I * (int64_t)sizeof(float));
}

int aura_stdp_update(const void* pre, const void* post, const float* x_in, const float* y_in, float* x_out,
                     float* y_out, float* W, float* dw_out, float lambda_pre, float lambda_post, float a_plus,
                     float a_minus, float lr, float w_min, float w_max, int64_t B, int64_t T, int64_t I, int64_t O,
                     int dtype, int flags, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!stdp_shape_ok(B, T, I, O)) return AURA_E_INVAL;
    if (dtype != AURA_DTYPE_F32 && dtype != AURA_DTYPE_BF16) return AURA_E_INVAL;
    if (flags & ~(AURA_STDP_PRE_TIME_INVARIANT | AURA_STDP_NO_APPLY)) return AURA_E_INVAL;
    if (I % 4 || O % 4) return AURA_E_INVAL;            // dW and W move as float4; the inputs are read per element
    const bool apply = !(flags & AURA_STDP_NO_APPLY);
    if (!pre || !post || !workspace) return AURA_E_INVAL;
    if (apply ? !W : !dw_out) return AURA_E_INVAL;
    if (!apply) W = nullptr;
    if (apply && !(w_min <= w_max)) return AURA_E_INVAL;
    // a trace that is read must not be the one that is written: other workgroups read the incoming value of a row
    if ((x_in && x_in == x_out) || (y_in && y_in == y_out)) return AURA_E_INVAL;
    const int64_t need = aura_stdp_workspace_bytes(B, T, I, O);
    if (workspace_bytes < need) return AURA_E_INVAL;
    if (misaligned(workspace, 256) || misaligned(pre, 16) || misaligned(post, 16) || misaligned(W, 16) ||
        misaligned(dw_out, 16) || misaligned(x_in, 4) || misaligned(y_in, 4) || misaligned(x_out, 4) ||
        misaligned(y_out, 4))
        return AURA_E_ALIGN;
    StdpArgs a;
    a.pre = pre; a.post = post; a.x_in = x_in; a.y_in = y_in; a.x_out = x_out; a.y_out = y_out;
    a.part = static_cast<float*>(workspace);
    a.lambda_pre = lambda_pre; a.lambda_post = lambda_post; a.a_plus = a_plus; a.neg_a_minus = -a_minus;
    a.B = B; a.T = T; a.I = I; a.O = O;
    a.splits = (int)stdp_splits(B, I, O);
    a.pre_invariant = (flags & AURA_STDP_PRE_TIME_INVARIANT) ? 1 : 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)stdp_tiles(I), (unsigned)stdp_tiles(O), (unsigned)a.splits), block(256);
    const bool bf16 = dtype == AURA_DTYPE_BF16;
    if (a.pre_invariant) {
        if (bf16) hipLaunchKernelGGL((stdp_partial_kernel<true, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((stdp_partial_kernel<false, true>), grid, block, 0, s, a);
    } else {
        if (bf16) hipLaunchKernelGGL((stdp_partial_kernel<true, false>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((stdp_partial_kernel<false, false>), grid, block, 0, s, a);
    }
    if (aura_check_launch() != AURA_OK) return AURA_E_LAUNCH;
    const int64_t n4 = O * I / 4;
    hipLaunchKernelGGL(stdp_finish_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, a.part, a.splits, n4,
                       (float)B, W, dw_out, lr, w_min, w_max);
    return aura_check_launch();
}

}  // extern "C"
