// aura_decode.hip -- one cached decoding step of HippocampalProsodyAttention: query modulation, K/V append and the new
// query row's attention over the cache, in a chunk launch and a merge launch (gfx950).
// The rule is stated once, in include/aura_hip.h ("Decode attention"); the comments here are about how it is computed.
//   chunk   one wave per (b, h, chunk of 256 positions), four waves per workgroup.  A K or V row is dh / 4 float4 units;
//           GP (the power of two >= dh / 4) lanes share a row, so a wave reads R = 64 / GP consecutive rows with one
//           16-byte load per lane: contiguous in memory, straight to registers, no LDS.  A slot keeps its own running
//           (m, l, acc) and takes four of its positions per update (eight loads in flight per lane); the slots are
//           merged by a symmetric butterfly.  The scale s is recomputed by every wave (x and wm are a few KB in L2).
//           Position L is read from k_new / v_new, never from the cache; the wave of chunk L / 256 writes it there.
//   merge   one wave per (b, h): the chunks in ascending order, ctx = acc / l, and lengths[b] += 1 by the wave of head 0.
//           The chunk count comes from the workspace header the chunk-0 wave wrote, so no wave of this launch reads a
//           length that another is advancing.
// No atomics; nothing depends on the batch, the capacity or the grid.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/aura_hip.h"
#include "aura_common.inl"

namespace {

constexpr int DEC_WAVES = 4;
constexpr int DEC_CHUNK = 256;          // positions per chunk
constexpr int DEC_BLOCK = 4;            // positions a slot takes per softmax update
constexpr int DEC_HDR = 4;              // floats of header per (b, h): chunk count (int32), s, 0, 0
constexpr int DEC_PART = 4;             // floats before a chunk's acc: m, l, 0, 0
constexpr int DEC_MAX_D = 2048;
constexpr int DEC_MAX_CAP = 32768;

struct DecodeArgs {
    const float* q;                     // [B][D]
    const float* k_new;                 // [B][D]
    const float* v_new;                 // [B][D]
    const float* x;                     // [B][D] (with wm)
    const float* prosody;               // [B][4] or NULL
    const float* Wp;                    // [H][4]
    const float* bp;                    // [H]
    const float* wm;                    // [D] or NULL
    const float* bm;                    // [1] or NULL
    int32_t* lengths;                   // [B]
    float* Kc;                          // [B][H][cap][dh]
    float* Vc;
    float* ws;                          // [B H][DEC_HDR + n_chunks (DEC_PART + dh)]
    float* ctx;                         // [B][D]
    float* scale;                       // [B][H] or NULL
    int64_t B;
    int H, dh, D, cap, n_chunks, advance;
    float isq;
};

__device__ __forceinline__ int64_t dec_stride(const DecodeArgs& a) {
    return DEC_HDR + (int64_t)a.n_chunks * (DEC_PART + a.dh);
}

__device__ __forceinline__ float dec_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

__device__ __forceinline__ float dec_wave_sum(float s) {
    s = s + __shfl_xor(s, 32);
    s = s + __shfl_xor(s, 16);
    s = s + __shfl_xor(s, 8);
    s = s + __shfl_xor(s, 4);
    s = s + __shfl_xor(s, 2);
    s = s + __shfl_xor(s, 1);
    return s;
}

// the query scale of (b, h); every lane of the wave takes part and gets the same bits
__device__ __forceinline__ float dec_scale(const DecodeArgs& a, int64_t b, int h, int lane) {
    float s = 1.0f;
    if (a.prosody) {
        const float* p = a.prosody + b * 4;
        const float* wp = a.Wp + h * 4;
        const float p0 = p[0], p1 = p[1];
        float g = wp[0] * p0;
        g = g + wp[1] * p1;
        g = g + wp[2] * p[2];
        g = g + wp[3] * p[3];
        g = g + a.bp[h];
        const float fp = 1.0f + dec_sigmoid(g);
        const float fa = 1.0f + 0.2f * tanhf(p0);
        const float fv = 1.0f + 0.05f * tanhf(p1);
        s = (fp * fa) * fv;
    }
    if (a.wm) {
        const float4* xr = reinterpret_cast<const float4*>(a.x + b * a.D);
        const float4* wr = reinterpret_cast<const float4*>(a.wm);
        const int U = a.D / 4;
        float d = 0.0f;
        for (int u = lane; u < U; u += 64) {
            const float4 xv = xr[u], wv = wr[u];
            d = d + wv.x * xv.x;
            d = d + wv.y * xv.y;
            d = d + wv.z * xv.z;
            d = d + wv.w * xv.w;
        }
        d = dec_wave_sum(d) + a.bm[0];
        s = s * (1.0f + 0.5f * dec_sigmoid(d));
    }
    return s;
}

__device__ __forceinline__ float4 dec_shfl4(const float4 v, int off) {
    return make_float4(__shfl_xor(v.x, off), __shfl_xor(v.y, off), __shfl_xor(v.z, off), __shfl_xor(v.w, off));
}

template <int GP>
__global__ __launch_bounds__(64 * DEC_WAVES) void attn_decode_chunk_kernel(const DecodeArgs a) {
    constexpr int R = 64 / GP;                                          // slots: rows a wave reads at once
    constexpr int PER_SLOT = DEC_CHUNK / R;                             // a multiple of DEC_BLOCK: R <= 64
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t w = (int64_t)blockIdx.x * DEC_WAVES + wave;
    if (w >= a.B * a.H * a.n_chunks) return;
    const int c = (int)(w % a.n_chunks);
    const int64_t bh = w / a.n_chunks;
    const int h = (int)(bh % a.H);
    const int64_t b = bh / a.H;
    const int L = a.lengths[b];
    const int lim = a.cap < DEC_CHUNK * a.n_chunks ? a.cap : DEC_CHUNK * a.n_chunks;
    float* const blk = a.ws + bh * dec_stride(a);
    if (L < 0 || L >= lim) {                                            // inactive: the merge writes the zeros
        if (c == 0 && lane == 0) {
            reinterpret_cast<int32_t*>(blk)[0] = 0;
            if (a.scale) a.scale[bh] = 0.0f;
        }
        return;
    }
    const int t0 = c * DEC_CHUNK;
    if (t0 > L) return;                                                 // the whole wave: no shuffle is skipped
    const int end = t0 + DEC_CHUNK < L + 1 ? t0 + DEC_CHUNK : L + 1;    // positions [t0, end), end <= L + 1 <= cap

    const float s = dec_scale(a, b, h, lane);
    const int G = a.dh / 4;
    const int j = lane % GP, r = lane / GP;
    const bool col = j < G;
    const int64_t row_new = (b * a.D + (int64_t)h * a.dh) / 4;           // float4 index of this head in a [B][D] row
    const float4* const kn = reinterpret_cast<const float4*>(a.k_new) + row_new;
    const float4* const vn = reinterpret_cast<const float4*>(a.v_new) + row_new;
    const int64_t base = bh * a.cap * G;                                // float4 index of Kc[b][h][0]; < 2^31 * 2^15 * 2^5
    float4* const K4 = reinterpret_cast<float4*>(a.Kc) + base;
    float4* const V4 = reinterpret_cast<float4*>(a.Vc) + base;

    float4 qv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (col) {
        qv = (reinterpret_cast<const float4*>(a.q) + row_new)[j];
        qv.x = qv.x * s; qv.y = qv.y * s; qv.z = qv.z * s; qv.w = qv.w * s;
    }

    float m = -INFINITY, l = 0.0f;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int i = 0; i < PER_SLOT; i += DEC_BLOCK) {
        if (t0 + R * i >= end) break;                                   // slot 0's first position of the block: uniform
        float4 kk[DEC_BLOCK], vv[DEC_BLOCK];
        bool ok[DEC_BLOCK];
#pragma unroll
        for (int u = 0; u < DEC_BLOCK; ++u) {
            const int t = t0 + r + R * (i + u);
            ok[u] = t < end;
            kk[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            vv[u] = kk[u];
            if (ok[u] && col) {
                const bool nw = t == L;                                 // the new position: from k_new / v_new
                const float4* const kp = nw ? kn + j : K4 + (int64_t)t * G + j;
                const float4* const vp = nw ? vn + j : V4 + (int64_t)t * G + j;
                kk[u] = *kp;
                vv[u] = *vp;
            }
        }
        float z[DEC_BLOCK];
        float mn = m;
#pragma unroll
        for (int u = 0; u < DEC_BLOCK; ++u) {
            float d = qv.x * kk[u].x;
            d = d + qv.y * kk[u].y;
            d = d + qv.z * kk[u].z;
            d = d + qv.w * kk[u].w;
#pragma unroll
            for (int off = GP / 2; off >= 1; off >>= 1) d = d + __shfl_xor(d, off);
            z[u] = d * a.isq;
            if (ok[u]) mn = fmaxf(mn, z[u]);
        }
        const float al = m == mn ? 1.0f : expf(m - mn);
        l = l * al;
        acc.x = acc.x * al; acc.y = acc.y * al; acc.z = acc.z * al; acc.w = acc.w * al;
#pragma unroll
        for (int u = 0; u < DEC_BLOCK; ++u) {
            if (ok[u]) {
                const float p = expf(z[u] - mn);
                l = l + p;
                acc.x = acc.x + p * vv[u].x;
                acc.y = acc.y + p * vv[u].y;
                acc.z = acc.z + p * vv[u].z;
                acc.w = acc.w + p * vv[u].w;
            }
        }
        m = mn;
    }

    // the slots of the chunk: a symmetric merge, so both partners hold the same bits
#pragma unroll
    for (int off = GP; off < 64; off <<= 1) {
        const float mo = __shfl_xor(m, off), lo = __shfl_xor(l, off);
        const float4 ao = dec_shfl4(acc, off);
        const float M = fmaxf(m, mo);
        const float ea = m == -INFINITY ? 0.0f : expf(m - M);
        const float eb = mo == -INFINITY ? 0.0f : expf(mo - M);
        l = l * ea + lo * eb;
        acc.x = acc.x * ea + ao.x * eb;
        acc.y = acc.y * ea + ao.y * eb;
        acc.z = acc.z * ea + ao.z * eb;
        acc.w = acc.w * ea + ao.w * eb;
        m = M;
    }

    if (r == 0 && col) {
        float4* const part = reinterpret_cast<float4*>(blk + DEC_HDR + (int64_t)c * (DEC_PART + a.dh));
        if (j == 0) part[0] = make_float4(m, l, 0.0f, 0.0f);
        part[1 + j] = acc;
        if (c == L / DEC_CHUNK) {                                       // the one wave of (b, h) that appends
            K4[(int64_t)L * G + j] = kn[j];
            V4[(int64_t)L * G + j] = vn[j];
        }
    }
    if (c == 0 && lane == 0) {
        reinterpret_cast<int32_t*>(blk)[0] = L / DEC_CHUNK + 1;
        blk[1] = s;
        if (a.scale) a.scale[bh] = s;
    }
}

__global__ __launch_bounds__(64 * DEC_WAVES) void attn_decode_merge_kernel(const DecodeArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t bh = (int64_t)blockIdx.x * DEC_WAVES + wave;
    if (bh >= a.B * a.H) return;
    const int h = (int)(bh % a.H);
    const int64_t b = bh / a.H;
    const float* const blk = a.ws + bh * dec_stride(a);
    const int nv = reinterpret_cast<const int32_t*>(blk)[0];            // 0: inactive; else <= n_chunks as written
    const int G = a.dh / 4;
    if (lane < G) {
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (nv > 0) {
            const float4* part = reinterpret_cast<const float4*>(blk + DEC_HDR);
            const int pstride = (DEC_PART + a.dh) / 4;
            float M = part[0].x, l = part[0].y;
            acc = part[1 + lane];
            for (int c = 1; c < nv; ++c) {
                part += pstride;
                const float4 hd = part[0], ac = part[1 + lane];
                const float Mn = fmaxf(M, hd.x);
                const float ea = expf(M - Mn), eb = expf(hd.x - Mn);
                l = l * ea + hd.y * eb;
                acc.x = acc.x * ea + ac.x * eb;
                acc.y = acc.y * ea + ac.y * eb;
                acc.z = acc.z * ea + ac.z * eb;
                acc.w = acc.w * ea + ac.w * eb;
                M = Mn;
            }
            acc.x = acc.x / l; acc.y = acc.y / l; acc.z = acc.z / l; acc.w = acc.w / l;
        }
        (reinterpret_cast<float4*>(a.ctx) + (b * a.D + (int64_t)h * a.dh) / 4)[lane] = acc;
    }
    if (a.advance && h == 0 && lane == 0 && nv > 0) a.lengths[b] = a.lengths[b] + 1;
}

// ---------------------------------------------------------------------------------------------------------- extend
// m new tokens per row in one pass over K and V (the rule: "Decode attention: extend").  The arguments are the step's
// with every [B] row array [B m] rows long (row b m + j is query j of sequence b), so dec_scale serves as it is.
//   chunk   one wave per (b, h, chunk, group of EXT_GROUP queries).  It loads a block of four positions per slot once
//           and updates the running (m, l, acc) of its queries from it, each with the step's operation sequence and no
//           branch between them, so that the queries' chains interleave; the groups of a chunk are separate waves (the
//           later ones hit L2).  Query j sees the positions < L + j + 1: a block past its end leaves its state alone.
//           Positions >= L are read from k_new / v_new, never from the cache; position L + j is appended by the wave
//           of chunk (L + j) / 256 and of j's group.
//   merge   one wave per (b, j, h), the step's merge; lengths[b] += m by the wave of j = 0, h = 0.
constexpr int EXT_GROUP = 8;            // queries that share a block's loads (register report: DESIGN 4.19)
constexpr int EXT_MAX_M = 32;

struct ExtendArgs {
    DecodeArgs d;                       // q, k_new, v_new, x, ctx [B m][D]; prosody [B m][4]; scale [B m][H]; ws per (b, j, h)
    int m;
};

// per-row counts ("a restriction of the rule"): row b takes its first counts[b] of the m padded query rows.  The kernels
// below are one text for both argument types; with ExtendArgs the row's count is m itself, a compile-time identity, so
// those instantiations are the code they were (register report: profiles/ragged_extend_kernels.json).
struct RaggedExtendArgs {
    DecodeArgs d;
    int m;
    const int32_t* counts;              // [B]
};

template <class Args> struct ext_ragged { static constexpr bool value = false; };
template <> struct ext_ragged<RaggedExtendArgs> { static constexpr bool value = true; };

__device__ __forceinline__ int ext_count(const ExtendArgs& e, int64_t) { return e.m; }
__device__ __forceinline__ int ext_count(const RaggedExtendArgs& e, int64_t b) { return e.counts[b]; }

template <int GP, class Args>
__global__ __launch_bounds__(64 * DEC_WAVES) void attn_extend_chunk_kernel(const Args e) {
    constexpr int R = 64 / GP;
    constexpr int PER_SLOT = DEC_CHUNK / R;
    constexpr bool RAGGED = ext_ragged<Args>::value;
    const DecodeArgs& a = e.d;
    const int m = e.m;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_groups = (m + EXT_GROUP - 1) / EXT_GROUP;
    const int64_t w = (int64_t)blockIdx.x * DEC_WAVES + wave;           // ((b H + h) n_chunks + c) n_groups + group
    if (w >= a.B * a.H * a.n_chunks * n_groups) return;
    const int g0 = (int)(w % n_groups) * EXT_GROUP;                     // the wave's queries: g0 .. g0 + EXT_GROUP - 1
    const int c = (int)((w / n_groups) % a.n_chunks);
    const int64_t bh = w / n_groups / a.n_chunks;
    const int h = (int)(bh % a.H);
    const int64_t b = bh / a.H;
    const int64_t row0 = b * m;                                         // the first of the sequence's m query rows
    const int L = a.lengths[b];
    const int lim = a.cap < DEC_CHUNK * a.n_chunks ? a.cap : DEC_CHUNK * a.n_chunks;
    const int64_t stride = dec_stride(a);
    const int mb = ext_count(e, b);                                     // the row's own count; m without counts
    // with counts the four tests are joined without short circuit, so that the count's load does not wait behind the
    // branch on the length: both loads are in flight together
    const bool inactive = RAGGED ? bool((L < 0) | (mb < 0) | (mb > m) | (L + mb > lim)) : (L < 0 || L + m > lim);
    if (inactive) {                                                     // the merge writes the zeros
        if (c == 0 && g0 == 0) {
            for (int q = lane; q < m; q += 64) {
                const int64_t rh = (row0 + q) * a.H + h;
                reinterpret_cast<int32_t*>(a.ws + rh * stride)[0] = 0;
                if (a.scale) a.scale[rh] = 0.0f;
            }
        }
        return;
    }
    if (RAGGED) {
        if (c == 0 && g0 == 0) {                                        // the padded queries: a header the merge can read
            for (int q = mb + lane; q < m; q += 64) {
                const int64_t rh = (row0 + q) * a.H + h;
                reinterpret_cast<int32_t*>(a.ws + rh * stride)[0] = 0;
                if (a.scale) a.scale[rh] = 0.0f;
            }
        }
        if (g0 >= mb) return;                                           // no query of the row in this group; the whole
    }                                                                   // wave, before any shuffle
    const int t0 = c * DEC_CHUNK;
    const int glast = (g0 + EXT_GROUP < mb ? g0 + EXT_GROUP : mb) - 1;
    if (t0 > L + glast) return;                                         // no query of the group reaches this chunk; the
                                                                        // whole wave: no shuffle is skipped

    const int G = a.dh / 4, D4 = a.D / 4;
    const int j = lane % GP, r = lane / GP;
    const bool col = j < G;
    const int64_t row_new = (row0 * a.D + (int64_t)h * a.dh) / 4;       // float4 index of this head in query row 0
    const float4* const kn = reinterpret_cast<const float4*>(a.k_new) + row_new;     // query row q: + q * D4
    const float4* const vn = reinterpret_cast<const float4*>(a.v_new) + row_new;
    const float4* const qn = reinterpret_cast<const float4*>(a.q) + row_new;
    const int64_t base = bh * a.cap * G;
    float4* const K4 = reinterpret_cast<float4*>(a.Kc) + base;
    float4* const V4 = reinterpret_cast<float4*>(a.Vc) + base;

    {
        const int gend = t0 + DEC_CHUNK < L + glast + 1 ? t0 + DEC_CHUNK : L + glast + 1;

        float4 qv[EXT_GROUP], acc[EXT_GROUP];
        float mx[EXT_GROUP], l[EXT_GROUP];
        int end[EXT_GROUP];                                             // query's positions here: [t0, end); t0: none
#pragma unroll
        for (int g = 0; g < EXT_GROUP; ++g) {
            const int q = g0 + g;
            qv[g] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            acc[g] = qv[g];
            mx[g] = -INFINITY;
            l[g] = 0.0f;
            end[g] = t0;
            if (q < mb && t0 <= L + q) {                                // uniform
                end[g] = t0 + DEC_CHUNK < L + q + 1 ? t0 + DEC_CHUNK : L + q + 1;
                const float s = dec_scale(a, row0 + q, h, lane);
                if (col) {
                    float4 v = qn[(int64_t)q * D4 + j];
                    v.x = v.x * s; v.y = v.y * s; v.z = v.z * s; v.w = v.w * s;
                    qv[g] = v;
                }
                if (c == 0 && lane == 0) {
                    const int64_t rh = (row0 + q) * a.H + h;
                    float* const blk = a.ws + rh * stride;
                    reinterpret_cast<int32_t*>(blk)[0] = (L + q) / DEC_CHUNK + 1;
                    blk[1] = s;
                    if (a.scale) a.scale[rh] = s;
                }
            }
        }

        for (int i = 0; i < PER_SLOT; i += DEC_BLOCK) {
            const int first = t0 + R * i;                               // slot 0's first position of the block
            if (first >= gend) break;
            float4 kk[DEC_BLOCK], vv[DEC_BLOCK];
            int tt[DEC_BLOCK];
#pragma unroll
            for (int u = 0; u < DEC_BLOCK; ++u) {
                const int t = first + r + R * u;
                tt[u] = t;
                kk[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                vv[u] = kk[u];
                if (t < gend && col) {
                    const bool nw = t >= L;                             // a new position: row t - L of k_new / v_new
                    const float4* const kp = nw ? kn + (int64_t)(t - L) * D4 + j : K4 + (int64_t)t * G + j;
                    const float4* const vp = nw ? vn + (int64_t)(t - L) * D4 + j : V4 + (int64_t)t * G + j;
                    kk[u] = *kp;
                    vv[u] = *vp;
                }
            }
#pragma unroll
            for (int g = 0; g < EXT_GROUP; ++g) {
                // no branch: the queries of a group are independent chains that the scheduler interleaves.  A block
                // in which a query has no position selects its old state back, bit for bit (al = 1).
                float z[DEC_BLOCK];
                float mn = mx[g];
#pragma unroll
                for (int u = 0; u < DEC_BLOCK; ++u) {
                    float d = qv[g].x * kk[u].x;
                    d = d + qv[g].y * kk[u].y;
                    d = d + qv[g].z * kk[u].z;
                    d = d + qv[g].w * kk[u].w;
#pragma unroll
                    for (int off = GP / 2; off >= 1; off >>= 1) d = d + __shfl_xor(d, off);
                    z[u] = d * a.isq;
                    mn = tt[u] < end[g] ? fmaxf(mn, z[u]) : mn;
                }
                const float al = mx[g] == mn ? 1.0f : expf(mx[g] - mn);
                l[g] = l[g] * al;
                acc[g].x = acc[g].x * al; acc[g].y = acc[g].y * al; acc[g].z = acc[g].z * al; acc[g].w = acc[g].w * al;
#pragma unroll
                for (int u = 0; u < DEC_BLOCK; ++u) {
                    const bool ok = tt[u] < end[g];
                    const float p = expf(z[u] - mn);
                    l[g] = ok ? l[g] + p : l[g];
                    acc[g].x = ok ? acc[g].x + p * vv[u].x : acc[g].x;
                    acc[g].y = ok ? acc[g].y + p * vv[u].y : acc[g].y;
                    acc[g].z = ok ? acc[g].z + p * vv[u].z : acc[g].z;
                    acc[g].w = ok ? acc[g].w + p * vv[u].w : acc[g].w;
                }
                mx[g] = mn;
            }
        }

#pragma unroll
        for (int g = 0; g < EXT_GROUP; ++g) {
            if (end[g] == t0) continue;                                 // uniform: not a query of this chunk
            float M0 = mx[g], l0 = l[g];
            float4 a0 = acc[g];
#pragma unroll
            for (int off = GP; off < 64; off <<= 1) {
                const float mo = __shfl_xor(M0, off), lo = __shfl_xor(l0, off);
                const float4 ao = dec_shfl4(a0, off);
                const float M = fmaxf(M0, mo);
                const float ea = M0 == -INFINITY ? 0.0f : expf(M0 - M);
                const float eb = mo == -INFINITY ? 0.0f : expf(mo - M);
                l0 = l0 * ea + lo * eb;
                a0.x = a0.x * ea + ao.x * eb;
                a0.y = a0.y * ea + ao.y * eb;
                a0.z = a0.z * ea + ao.z * eb;
                a0.w = a0.w * ea + ao.w * eb;
                M0 = M;
            }
            if (r == 0 && col) {
                const int64_t rh = (row0 + g0 + g) * a.H + h;
                float4* const part = reinterpret_cast<float4*>(a.ws + rh * stride + DEC_HDR +
                                                               (int64_t)c * (DEC_PART + a.dh));
                if (j == 0) part[0] = make_float4(M0, l0, 0.0f, 0.0f);
                part[1 + j] = a0;
            }
        }
    }

    // the append of the group's own positions: slot r takes L + g0 + r, L + g0 + r + R, ..; each belongs to exactly one
    // chunk, and the wave of that chunk and this group has not returned above
    if (col) {
        for (int q = g0 + r; q <= glast; q += R) {
            if ((L + q) / DEC_CHUNK == c) {
                K4[(int64_t)(L + q) * G + j] = kn[(int64_t)q * D4 + j];
                V4[(int64_t)(L + q) * G + j] = vn[(int64_t)q * D4 + j];
            }
        }
    }
}

template <class Args>
__global__ __launch_bounds__(64 * DEC_WAVES) void attn_extend_merge_kernel(const Args e) {
    const DecodeArgs& a = e.d;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t rh = (int64_t)blockIdx.x * DEC_WAVES + wave;          // (b m + j) H + h
    if (rh >= a.B * e.m * a.H) return;
    const int h = (int)(rh % a.H);
    const int64_t row = rh / a.H;
    const float* const blk = a.ws + rh * dec_stride(a);
    const int nv = reinterpret_cast<const int32_t*>(blk)[0];            // 0: inactive; else <= n_chunks as written
    const int G = a.dh / 4;
    if (lane < G) {
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (nv > 0) {
            const float4* part = reinterpret_cast<const float4*>(blk + DEC_HDR);
            const int pstride = (DEC_PART + a.dh) / 4;
            float M = part[0].x, l = part[0].y;
            acc = part[1 + lane];
            for (int c = 1; c < nv; ++c) {
                part += pstride;
                const float4 hd = part[0], ac = part[1 + lane];
                const float Mn = fmaxf(M, hd.x);
                const float ea = expf(M - Mn), eb = expf(hd.x - Mn);
                l = l * ea + hd.y * eb;
                acc.x = acc.x * ea + ac.x * eb;
                acc.y = acc.y * ea + ac.y * eb;
                acc.z = acc.z * ea + ac.z * eb;
                acc.w = acc.w * ea + ac.w * eb;
                M = Mn;
            }
            acc.x = acc.x / l; acc.y = acc.y / l; acc.z = acc.z / l; acc.w = acc.w / l;
        }
        (reinterpret_cast<float4*>(a.ctx) + (row * a.D + (int64_t)h * a.dh) / 4)[lane] = acc;
    }
    if (a.advance && h == 0 && row % e.m == 0 && lane == 0 && nv > 0) {
        const int64_t b = row / e.m;
        a.lengths[b] = a.lengths[b] + ext_count(e, b);                  // nv > 0 at j = 0: active, count >= 1
    }
}

inline bool misaligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) != 0; }

// everything but the capacity: what the workspace's size depends on
inline bool dec_shape_ok(int64_t B, int64_t H, int64_t dh, int64_t n_chunks) {
    if (B < 0 || B > 0x7fffffff || H < 1 || dh < 4 || dh > 128 || dh % 4 != 0 || H * dh > DEC_MAX_D) return false;
    if (n_chunks < 1 || n_chunks * DEC_CHUNK > DEC_MAX_CAP + DEC_CHUNK - 1) return false;
    return B * H * n_chunks <= 0x7fffffff;                              // < 2^31 * 2^9 * 2^7: no overflow
}

inline int64_t dec_workspace_floats(int64_t B, int64_t H, int64_t dh, int64_t n_chunks) {
    return B * H * (DEC_HDR + n_chunks * (DEC_PART + dh));
}

inline void ext_set_counts(ExtendArgs&, const int32_t*) {}
inline void ext_set_counts(RaggedExtendArgs& e, const int32_t* counts) { e.counts = counts; }

// the extend's validation and its two launches, for either argument type
template <class Args>
int ext_launch(const float* q, const float* k_new, const float* v_new, const float* x, const float* prosody_or_null,
               const float* Wp, const float* bp, const float* wm_or_null, const float* bm_or_null, int32_t* lengths,
               const int32_t* counts, float* Kc, float* Vc, int64_t B, int64_t m, int64_t H, int64_t dh, int64_t cap,
               int64_t n_chunks, int advance, float* workspace, int64_t workspace_bytes, float* ctx,
               float* scale_or_null, void* stream) {
    if (!dec_shape_ok(B, H, dh, n_chunks) || m < 1 || m > EXT_MAX_M) return AURA_E_INVAL;
    if (B * m * H * n_chunks > 0x7fffffff) return AURA_E_INVAL;         // < 2^31 * 2^5 * 2^9 * 2^8: no overflow
    if (cap < 1 || cap > DEC_MAX_CAP || n_chunks * DEC_CHUNK > cap + DEC_CHUNK - 1) return AURA_E_INVAL;
    if (!q || !k_new || !v_new || !lengths || !Kc || !Vc || !workspace || !ctx) return AURA_E_INVAL;
    if (prosody_or_null && (!Wp || !bp)) return AURA_E_INVAL;
    if ((wm_or_null == nullptr) != (bm_or_null == nullptr) || (wm_or_null && !x)) return AURA_E_INVAL;
    if (workspace_bytes < dec_workspace_floats(B * m, H, dh, n_chunks) * 4) return AURA_E_INVAL;
    if (misaligned(q, 16) || misaligned(k_new, 16) || misaligned(v_new, 16) || misaligned(x, 16) ||
        misaligned(wm_or_null, 16) || misaligned(Kc, 16) || misaligned(Vc, 16) || misaligned(workspace, 16) ||
        misaligned(ctx, 16) || misaligned(prosody_or_null, 4) || misaligned(Wp, 4) || misaligned(bp, 4) ||
        misaligned(bm_or_null, 4) || misaligned(lengths, 4) || misaligned(scale_or_null, 4))
        return AURA_E_ALIGN;
    if (B == 0) return AURA_OK;
    Args e;
    DecodeArgs& a = e.d;
    a.q = q; a.k_new = k_new; a.v_new = v_new; a.x = x; a.prosody = prosody_or_null; a.Wp = Wp; a.bp = bp;
    a.wm = wm_or_null; a.bm = bm_or_null; a.lengths = lengths; a.Kc = Kc; a.Vc = Vc; a.ws = workspace; a.ctx = ctx;
    a.scale = scale_or_null;
    a.B = B; a.H = (int)H; a.dh = (int)dh; a.D = (int)(H * dh); a.cap = (int)cap; a.n_chunks = (int)n_chunks;
    a.advance = advance != 0;
    a.isq = 1.0f / sqrtf((float)dh);
    e.m = (int)m;
    ext_set_counts(e, counts);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 block(64 * DEC_WAVES);
    const int64_t n_groups = (m + EXT_GROUP - 1) / EXT_GROUP;           // B H n_chunks n_groups <= B m H n_chunks
    const dim3 grid((unsigned)((B * H * n_chunks * n_groups + DEC_WAVES - 1) / DEC_WAVES));
    const int G = (int)dh / 4;
#define EXT_CHUNK_LAUNCH(GP) hipLaunchKernelGGL((attn_extend_chunk_kernel<GP, Args>), grid, block, 0, s, e)
    if (G <= 1) EXT_CHUNK_LAUNCH(1); else if (G <= 2) EXT_CHUNK_LAUNCH(2); else if (G <= 4) EXT_CHUNK_LAUNCH(4);
    else if (G <= 8) EXT_CHUNK_LAUNCH(8); else if (G <= 16) EXT_CHUNK_LAUNCH(16); else EXT_CHUNK_LAUNCH(32);
#undef EXT_CHUNK_LAUNCH
    hipLaunchKernelGGL((attn_extend_merge_kernel<Args>), dim3((unsigned)((B * m * H + DEC_WAVES - 1) / DEC_WAVES)), block,
                       0, s, e);
    return aura_check_launch();
}

}  // namespace

extern "C" {

int64_t aura_attn_decode_workspace_bytes(int64_t B, int64_t H, int64_t dh, int64_t n_chunks) {
    if (!dec_shape_ok(B, H, dh, n_chunks)) return -1;
    const int64_t bytes = dec_workspace_floats(B, H, dh, n_chunks) * 4;
    return bytes < 16 ? 16 : bytes;
}

int aura_attn_decode_step(const float* q, const float* k_new, const float* v_new, const float* x,
                          const float* prosody_or_null, const float* Wp, const float* bp, const float* wm_or_null,
                          const float* bm_or_null, int32_t* lengths, float* Kc, float* Vc, int64_t B, int64_t H,
                          int64_t dh, int64_t cap, int64_t n_chunks, int advance, float* workspace,
                          int64_t workspace_bytes, float* ctx, float* scale_or_null, void* stream) {
    if (!dec_shape_ok(B, H, dh, n_chunks)) return AURA_E_INVAL;
    if (cap < 1 || cap > DEC_MAX_CAP || n_chunks * DEC_CHUNK > cap + DEC_CHUNK - 1) return AURA_E_INVAL;
    if (!q || !k_new || !v_new || !lengths || !Kc || !Vc || !workspace || !ctx) return AURA_E_INVAL;
    if (prosody_or_null && (!Wp || !bp)) return AURA_E_INVAL;
    if ((wm_or_null == nullptr) != (bm_or_null == nullptr) || (wm_or_null && !x)) return AURA_E_INVAL;
    if (workspace_bytes < dec_workspace_floats(B, H, dh, n_chunks) * 4) return AURA_E_INVAL;
    if (misaligned(q, 16) || misaligned(k_new, 16) || misaligned(v_new, 16) || misaligned(x, 16) ||
        misaligned(wm_or_null, 16) || misaligned(Kc, 16) || misaligned(Vc, 16) || misaligned(workspace, 16) ||
        misaligned(ctx, 16) || misaligned(prosody_or_null, 4) || misaligned(Wp, 4) || misaligned(bp, 4) ||
        misaligned(bm_or_null, 4) || misaligned(lengths, 4) || misaligned(scale_or_null, 4))
        return AURA_E_ALIGN;
    if (B == 0) return AURA_OK;
    DecodeArgs a;
    a.q = q; a.k_new = k_new; a.v_new = v_new; a.x = x; a.prosody = prosody_or_null; a.Wp = Wp; a.bp = bp;
    a.wm = wm_or_null; a.bm = bm_or_null; a.lengths = lengths; a.Kc = Kc; a.Vc = Vc; a.ws = workspace; a.ctx = ctx;
    a.scale = scale_or_null;
    a.B = B; a.H = (int)H; a.dh = (int)dh; a.D = (int)(H * dh); a.cap = (int)cap; a.n_chunks = (int)n_chunks;
    a.advance = advance != 0;
    a.isq = 1.0f / sqrtf((float)dh);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 block(64 * DEC_WAVES);
    const dim3 grid((unsigned)((B * H * n_chunks + DEC_WAVES - 1) / DEC_WAVES));
    const int G = (int)dh / 4;
#define DEC_CHUNK_LAUNCH(GP) hipLaunchKernelGGL((attn_decode_chunk_kernel<GP>), grid, block, 0, s, a)
    if (G <= 1) DEC_CHUNK_LAUNCH(1); else if (G <= 2) DEC_CHUNK_LAUNCH(2); else if (G <= 4) DEC_CHUNK_LAUNCH(4);
    else if (G <= 8) DEC_CHUNK_LAUNCH(8); else if (G <= 16) DEC_CHUNK_LAUNCH(16); else DEC_CHUNK_LAUNCH(32);
#undef DEC_CHUNK_LAUNCH
    hipLaunchKernelGGL(attn_decode_merge_kernel, dim3((unsigned)((B * H + DEC_WAVES - 1) / DEC_WAVES)), block, 0, s, a);
    return aura_check_launch();
}

int64_t aura_attn_decode_extend_workspace_bytes(int64_t B, int64_t m, int64_t H, int64_t dh, int64_t n_chunks) {
    if (!dec_shape_ok(B, H, dh, n_chunks) || m < 1 || m > EXT_MAX_M || B * m * H * n_chunks > 0x7fffffff) return -1;
    const int64_t bytes = dec_workspace_floats(B * m, H, dh, n_chunks) * 4;
    return bytes < 16 ? 16 : bytes;
}

int aura_attn_decode_extend(const float* q, const float* k_new, const float* v_new, const float* x,
                            const float* prosody_or_null, const float* Wp, const float* bp, const float* wm_or_null,
                            const float* bm_or_null, int32_t* lengths, float* Kc, float* Vc, int64_t B, int64_t m,
                            int64_t H, int64_t dh, int64_t cap, int64_t n_chunks, int advance, float* workspace,
                            int64_t workspace_bytes, float* ctx, float* scale_or_null, void* stream) {
    return ext_launch<ExtendArgs>(q, k_new, v_new, x, prosody_or_null, Wp, bp, wm_or_null, bm_or_null, lengths, nullptr,
                                  Kc, Vc, B, m, H, dh, cap, n_chunks, advance, workspace, workspace_bytes, ctx,
                                  scale_or_null, stream);
}

int aura_attn_decode_extend_counts(const float* q, const float* k_new, const float* v_new, const float* x,
                                   const float* prosody_or_null, const float* Wp, const float* bp,
                                   const float* wm_or_null, const float* bm_or_null, int32_t* lengths,
                                   const int32_t* counts, float* Kc, float* Vc, int64_t B, int64_t m, int64_t H,
                                   int64_t dh, int64_t cap, int64_t n_chunks, int advance, float* workspace,
                                   int64_t workspace_bytes, float* ctx, float* scale_or_null, void* stream) {
    if (!counts) return AURA_E_INVAL;
    if (misaligned(counts, 4)) return AURA_E_ALIGN;
    return ext_launch<RaggedExtendArgs>(q, k_new, v_new, x, prosody_or_null, Wp, bp, wm_or_null, bm_or_null, lengths,
                                        counts, Kc, Vc, B, m, H, dh, cap, n_chunks, advance, workspace, workspace_bytes,
                                        ctx, scale_or_null, stream);
}

}  // extern "C"
