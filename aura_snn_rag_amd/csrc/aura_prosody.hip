// aura_prosody.hip -- prosody attention: channels from token ids, the three-channel LIF scan, salience, smoothing,
// normalisation, exact k-winner selection and the gains in one launch (gfx950).
// The rule is stated once, in include/aura_hip.h ("Prosody attention"); the comments here are about how it is computed.
//   rows       one wave owns a row from its ids (or its given channels) to its outputs.  A workgroup is four waves = four
//              rows that share nothing (one wave when S > 2048, for the LDS), so there is no workgroup barrier and a wave
//              beyond the last row simply leaves.
//   chunks     the row is walked in chunks of 256 positions.  Per chunk: (1) lane-parallel, position t = 64 q + lane:
//              the ids are loaded coalesced, sinf / cosf (accurate, full range reduction) give the three channels, which
//              go to the wave's LDS tile [3][256] (and to `channels` when asked); (2) the membrane chain: lane c < 3
//              owns channel c, reads its tile row 16 bytes at a time (the next read is issued before the four steps of
//              the current one), runs mul, add, compare, select from registers and writes the four spikes back over the
//              inputs; the three channels advance in the same instructions; (3) lane-parallel again: spikes out, the
//              salience of the position into the wave's LDS row.  Nothing is re-read from memory per step.
//   row        the salience row [S] lives in LDS from then on: smoothing (a block of 64 positions is written one block
//              late, after every raw value it would overwrite has been read), the maximum (an xor butterfly: order-free),
//              the division, the selection and the write-out all read it there.
//   selection  the monotone key and the ballot bisection of aura_place.hip: the k-th largest key T in 32 steps, keys
//              above T win, of the keys equal to T the first in position order.  The keys of the first 2048 positions
//              are formed once and held in registers (32 per lane; groups of four blocks beyond the row are skipped by
//              a uniform branch); a longer row forms the rest from the LDS row in every step.  The winners are
//              compacted in position order, then ranked (value first, position second) by counting, k^2 / 64 compares
//              per lane; their values are added in rank order by every lane alike.
// LDS per wave: 4 (3 * 256 + ceil64(S) + 3 * 256) bytes: 8 KB at S = 512, 38 KB at S = 8192.  A wave's LDS operations
// execute in program order, so what some lanes write is read by others after a compiler fence only.
// No atomics anywhere; nothing depends on B, on the grid or on the device.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/aura_hip.h"
#include "aura_common.inl"

namespace {

constexpr int PROS_MAX_S = 8192;
constexpr int PROS_MAX_K = 256;
constexpr int PROS_MAX_M = 64;
constexpr int PROS_SLOTS = PROS_MAX_K / 64;
constexpr int PROS_CHUNK = 256;         // positions per pass of the chain
constexpr int PROS_WIDE_S = 2048;       // above this a workgroup is one wave
constexpr int PROS_REG_BLOCKS = 32;     // blocks of 64 positions whose selection keys a lane holds in registers

struct ProsodyArgs {
    const void* ids;                    // [B][S] int64 / int32, or NULL: the three channels are given
    const float* amp;                   // [B][S] each (ids == NULL)
    const float* pitch;
    const float* bound;
    const int32_t* lengths;             // [B] or NULL
    const float* v0;                    // [B][3] or NULL
    const float* decay;                 // [3]
    const float* weights;               // [3]
    float* gains;                       // [B][S]
    float* salience;                    // [B][S]
    float* mu;                          // [B]
    int32_t* winners;                   // [B][k]
    float* v_out;                       // [B][3]
    float* spikes;                      // [3][B][S] or NULL
    float* channels;                    // [3][B][S] or NULL
    int64_t B;
    int S, k, m;
    int id64, normalize, channels_only;
    float gain_up, min_gain, max_gain;
};

__device__ __forceinline__ uint32_t pros_key(float z) {
    uint32_t u = __float_as_uint(z);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;            // NaN: above +inf, all equal
    if (u == 0x80000000u) u = 0u;                                        // -0 is +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint64_t pros_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ int pros_count(uint64_t m) { return __builtin_popcountll(m); }
__device__ __forceinline__ int pros_prefix(uint64_t m) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
__device__ __forceinline__ void pros_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// f(j, key) for every block j < nlive of the row, ascending: the first PROS_REG_BLOCKS keys from registers (in groups
// of four, a group beyond the row skipped by a uniform branch), the rest formed from the LDS row
template <typename F>
__device__ __forceinline__ void pros_for_keys(const uint32_t (&rk)[PROS_REG_BLOCKS], const float* s_sal, int nlive,
                                              int len, int lane, F&& f) {
#pragma unroll
    for (int g = 0; g < PROS_REG_BLOCKS; g += 4) {
        if (g < nlive) {                                                 // uniform over the wave
#pragma unroll
            for (int j = g; j < g + 4; ++j) f(j, rk[j]);
        }
    }
    for (int g = PROS_REG_BLOCKS; g < nlive; g += 4) {                   // four reads in flight; a block beyond the
        uint32_t key[4];                                                 // row holds key 0, which no f acts on
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = (g + i) * 64 + lane;
            key[i] = t < len ? pros_key(s_sal[t]) : 0u;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) f(g + i, key[i]);
    }
}

// one step of the rule's LIF: v = fl(fl(d v) + x); s = v >= 1; v = fl(v - s)
__device__ __forceinline__ float pros_step(float& v, float d, float x) {
    v = d * v + x;
    const bool f = v >= 1.0f;
    v = f ? v - 1.0f : v;
    return f ? 1.0f : 0.0f;
}

__global__ __launch_bounds__(256) void prosody_attention_kernel(const ProsodyArgs a) {
    extern __shared__ __align__(16) float s_mem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
    if (b >= a.B) return;
    const int S = a.S, k = a.k;
    const int S_pad = (S + 63) & ~63;
    float* const s_x = s_mem + (size_t)wave * (3 * PROS_CHUNK + S_pad + 3 * PROS_MAX_K);   // [3][PROS_CHUNK]
    float* const s_sal = s_x + 3 * PROS_CHUNK;                                             // [S_pad]
    int* const s_idx = reinterpret_cast<int*>(s_sal + S_pad);                              // [PROS_MAX_K]
    float* const s_val = reinterpret_cast<float*>(s_idx + PROS_MAX_K);
    float* const s_rank = s_val + PROS_MAX_K;

    int len = a.lengths ? a.lengths[b] : S;
    len = len < 0 ? 0 : (len > S ? S : len);
    const int64_t row = b * S;
    const int64_t BS = a.B * S;

    // ---- channels, chain, salience: chunk by chunk
    const int c = lane < 3 ? lane : 2;
    float d = 0.0f, v = 0.0f;
    if (!a.channels_only) {
        d = a.decay[c];
        v = a.v0 ? a.v0[b * 3 + c] : 0.0f;
    }
    const float w0 = a.channels_only ? 0.0f : a.weights[0], w1 = a.channels_only ? 0.0f : a.weights[1],
                w2 = a.channels_only ? 0.0f : a.weights[2];
#pragma unroll 1
    for (int c0 = 0; c0 < S_pad; c0 += PROS_CHUNK) {
        float x0[4], x1[4], x2[4];
        if (a.ids) {
            float f[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int t = c0 + q * 64 + lane;
                f[q] = 0.0f;
                if (t < S)
                    f[q] = a.id64 ? (float)reinterpret_cast<const int64_t*>(a.ids)[row + t]
                                  : (float)reinterpret_cast<const int32_t*>(a.ids)[row + t];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                x0[q] = fabsf(sinf(f[q] * 0.1f));
                x1[q] = fabsf(cosf(f[q] * 0.05f));
                x2[q] = sinf(f[q] * 0.3f) > 0.8f ? 1.0f : 0.0f;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int t = c0 + q * 64 + lane;
                x0[q] = x1[q] = x2[q] = 0.0f;
                if (t < S) {
                    x0[q] = a.amp[row + t];
                    x1[q] = a.pitch[row + t];
                    x2[q] = a.bound[row + t];
                }
            }
        }
        if (a.channels) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int t = c0 + q * 64 + lane;
                if (t < S) {
                    a.channels[row + t] = x0[q];
                    a.channels[BS + row + t] = x1[q];
                    a.channels[2 * BS + row + t] = x2[q];
                }
            }
        }
        if (a.channels_only) continue;                                   // uniform over the grid
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            s_x[q * 64 + lane] = x0[q];
            s_x[PROS_CHUNK + q * 64 + lane] = x1[q];
            s_x[2 * PROS_CHUNK + q * 64 + lane] = x2[q];
        }
        pros_wave_sync();

        // the chain: lane c < 3 advances channel c over the live positions of the chunk
        const int n_live = len - c0 < PROS_CHUNK ? len - c0 : PROS_CHUNK;   // may be <= 0
        if (lane < 3 && n_live > 0) {
            float* const xs = s_x + lane * PROS_CHUNK;
            int t = 0;
            float4 x = *reinterpret_cast<const float4*>(xs);
#pragma unroll 2
            for (; t + 4 <= n_live; t += 4) {
                const float4 nx = *reinterpret_cast<const float4*>(xs + ((t + 4) & (PROS_CHUNK - 1)));
                float4 s;
                s.x = pros_step(v, d, x.x);
                s.y = pros_step(v, d, x.y);
                s.z = pros_step(v, d, x.z);
                s.w = pros_step(v, d, x.w);
                *reinterpret_cast<float4*>(xs + t) = s;
                x = nx;
            }
            for (; t < n_live; ++t) xs[t] = pros_step(v, d, xs[t]);
        }
        pros_wave_sync();

#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int t = c0 + q * 64 + lane;
            if (c0 + q * 64 < S_pad) {                                   // uniform over the wave
                const bool live = t < len;
                const float s0 = live ? s_x[q * 64 + lane] : 0.0f;
                const float s1 = live ? s_x[PROS_CHUNK + q * 64 + lane] : 0.0f;
                const float s2 = live ? s_x[2 * PROS_CHUNK + q * 64 + lane] : 0.0f;
                if (a.spikes && t < S) {
                    a.spikes[row + t] = s0;
                    a.spikes[BS + row + t] = s1;
                    a.spikes[2 * BS + row + t] = s2;
                }
                s_sal[t] = live ? (w0 * s0 + w1 * s1) + w2 * s2 : 0.0f;
            }
        }
        pros_wave_sync();
    }
    if (a.channels_only) return;
    if (lane < 3) a.v_out[b * 3 + lane] = v;

    const int nblk = S_pad >> 6;
    const int nlive = (len + 63) >> 6;                                   // blocks that hold a live position

    // ---- smoothing: block j is written after block j + 1 was computed from the raw values
    if (a.m > 1) {
        const int m = a.m, h = m >> 1;
        const float kw = 1.0f / (float)m;
        float prev = 0.0f;
        for (int j = 0; j < nlive; ++j) {
            const int t = j * 64 + lane;
            float acc = 0.0f;
            for (int i = 0; i < m; ++i) {
                const int u = t - h + i;
                const float p = (u >= 0 && u < len) ? kw * s_sal[u] : 0.0f;
                acc = i == 0 ? p : acc + p;
            }
            pros_wave_sync();
            if (j > 0) s_sal[t - 64] = prev;
            pros_wave_sync();
            prev = t < len ? acc : 0.0f;
        }
        if (nlive > 0) s_sal[(nlive - 1) * 64 + lane] = prev;
        pros_wave_sync();
    }

    // ---- normalisation by the row's maximum
    if (a.normalize && len > 0) {
        float mx = -INFINITY;
#pragma unroll 4
        for (int j = 0; j < nlive; ++j) {
            const int t = j * 64 + lane;
            if (t < len) mx = fmaxf(mx, s_sal[t]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 8));
        mx = fmaxf(mx, __shfl_xor(mx, 4));
        mx = fmaxf(mx, __shfl_xor(mx, 2));
        mx = fmaxf(mx, __shfl_xor(mx, 1));
        const float den = mx + 1e-6f;
#pragma unroll 4
        for (int j = 0; j < nlive; ++j) {
            const int t = j * 64 + lane;
            if (t < len) s_sal[t] = s_sal[t] / den;
        }
        pros_wave_sync();
    }

    // ---- the k_eff winners in rank order, their mean
    const int k_eff = k < len ? k : len;
    float avg = 0.0f;
    if (k_eff > 0) {
        // the keys of the first PROS_REG_BLOCKS blocks sit in registers; a longer row reads the rest from LDS
        uint32_t rk[PROS_REG_BLOCKS];
#pragma unroll
        for (int j = 0; j < PROS_REG_BLOCKS; ++j) {
            const int t = j * 64 + lane;
            rk[j] = t < len ? pros_key(s_sal[t]) : 0u;                   // 0: below every real key
        }
        const auto keys = [&](auto&& f) {
            pros_for_keys(rk, s_sal, nlive, len, lane, f);
        };
        uint32_t T = 0u;
#pragma unroll 1
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t cand = T | (1u << bit);
            int cnt = 0;
            keys([&](int, uint32_t key) { cnt += pros_count(pros_ballot(key >= cand)); });
            if (cnt >= k_eff) T = cand;
        }
        int above = 0;
        keys([&](int, uint32_t key) { above += pros_count(pros_ballot(key > T)); });
        const int need = k_eff - above;                                  // of the keys equal to T, in position order
        int eq_base = 0, w_base = 0;
        keys([&](int j, uint32_t key) {
            const bool is_eq = key == T;
            const uint64_t beq = pros_ballot(is_eq);
            const bool win = key > T || (is_eq && eq_base + pros_prefix(beq) < need);
            const uint64_t bw = pros_ballot(win);
            if (win) {
                const int pos = w_base + pros_prefix(bw);                // < k_eff: exactly k_eff positions win
                if (pos < PROS_MAX_K) {
                    s_idx[pos] = j * 64 + lane;
                    s_val[pos] = s_sal[j * 64 + lane];
                }
            }
            eq_base += pros_count(beq);
            w_base += pros_count(bw);
        });
        pros_wave_sync();
        // rank of list entry r: the entries with a larger key, and those with an equal key earlier in the list
#pragma unroll
        for (int s = 0; s < PROS_SLOTS; ++s) {
            const int r = s * 64 + lane;
            if (r < k_eff) {
                const float mine = s_val[r];
                const uint32_t mk = pros_key(mine);
                int rank = 0;
                for (int q = 0; q < k_eff; ++q) {
                    const uint32_t qk = pros_key(s_val[q]);
                    rank += (qk > mk || (qk == mk && q < r)) ? 1 : 0;
                }
                a.winners[b * k + rank] = s_idx[r];
                s_rank[rank] = mine;
            }
        }
        pros_wave_sync();
        float sum = s_rank[0];
        for (int q = 1; q < k_eff; ++q) sum = sum + s_rank[q];
        avg = sum / (float)k_eff;
    }
#pragma unroll
    for (int s = 0; s < PROS_SLOTS; ++s) {
        const int r = s * 64 + lane;
        if (r >= k_eff && r < k) a.winners[b * k + r] = -1;
    }

    // ---- gains
    const float range = a.max_gain - a.min_gain;
    const float mu = a.min_gain + range * tanhf(a.gain_up * avg);
    if (lane == 0) a.mu[b] = mu;
#pragma unroll 4
    for (int j = 0; j < nblk; ++j) {
        const int t = j * 64 + lane;
        if (t < S) {
            const float sal = s_sal[t];
            a.salience[row + t] = sal;
            a.gains[row + t] = mu * (1.0f + sal);
        }
    }
}

inline bool misaligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) != 0; }

}  // namespace

extern "C" {

int aura_prosody_attention(const void* ids_or_null, int id_bytes, const float* amp, const float* pitch,
                           const float* boundary, const int32_t* lengths_or_null, const float* v0_or_null,
                           const float* decay, const float* weights, float gain_up, float min_gain, float max_gain,
                           int smoothing, int normalize, int64_t B, int64_t S, int64_t k, float* gains, float* salience,
                           float* mu, int32_t* winners, float* v_out, float* spikes_or_null, float* channels_or_null,
                           void* stream) {
    if (B < 0 || B > 0x7fffffff || S < 1 || S > PROS_MAX_S) return AURA_E_INVAL;
    const int n_ch = (amp != nullptr) + (pitch != nullptr) + (boundary != nullptr);
    if (ids_or_null) {
        if (n_ch != 0 || (id_bytes != 8 && id_bytes != 4)) return AURA_E_INVAL;
    } else if (n_ch != 3 || id_bytes != 0) {
        return AURA_E_INVAL;
    }
    const int n_out = (gains != nullptr) + (salience != nullptr) + (mu != nullptr) + (winners != nullptr) +
                      (v_out != nullptr);
    if (n_out != 0 && n_out != 5) return AURA_E_INVAL;
    const bool channels_only = n_out == 0;
    if (channels_only) {
        if (!channels_or_null || spikes_or_null || lengths_or_null || v0_or_null) return AURA_E_INVAL;
    } else {
        if (k < 1 || k > PROS_MAX_K || k > S || smoothing < 1 || smoothing > PROS_MAX_M) return AURA_E_INVAL;
        if (!decay || !weights) return AURA_E_INVAL;
    }
    if (misaligned(ids_or_null, id_bytes == 8 ? 8 : 4) || misaligned(amp, 4) || misaligned(pitch, 4) ||
        misaligned(boundary, 4) || misaligned(lengths_or_null, 4) || misaligned(v0_or_null, 4) || misaligned(decay, 4) ||
        misaligned(weights, 4) || misaligned(gains, 4) || misaligned(salience, 4) || misaligned(mu, 4) ||
        misaligned(winners, 4) || misaligned(v_out, 4) || misaligned(spikes_or_null, 4) ||
        misaligned(channels_or_null, 4))
        return AURA_E_ALIGN;
    if (B == 0) return AURA_OK;
    ProsodyArgs a;
    a.ids = ids_or_null; a.amp = amp; a.pitch = pitch; a.bound = boundary; a.lengths = lengths_or_null;
    a.v0 = v0_or_null; a.decay = decay; a.weights = weights; a.gains = gains; a.salience = salience; a.mu = mu;
    a.winners = winners; a.v_out = v_out; a.spikes = spikes_or_null; a.channels = channels_or_null;
    a.B = B; a.S = (int)S; a.k = channels_only ? 1 : (int)k; a.m = channels_only ? 1 : smoothing;
    a.id64 = id_bytes == 8; a.normalize = normalize != 0; a.channels_only = channels_only;
    a.gain_up = gain_up; a.min_gain = min_gain; a.max_gain = max_gain;
    const int waves = S > PROS_WIDE_S ? 1 : 4;
    const int S_pad = ((int)S + 63) & ~63;
    const size_t lds = (size_t)waves * (3 * PROS_CHUNK + S_pad + 3 * PROS_MAX_K) * sizeof(float);   // <= 57344
    const dim3 grid((unsigned)((B + waves - 1) / waves)), block(64 * waves);
    hipLaunchKernelGGL(prosody_attention_kernel, grid, block, lds, static_cast<hipStream_t>(stream), a);
    return aura_check_launch();
}

}  // extern "C"
