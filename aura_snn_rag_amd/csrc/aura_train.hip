// aura_train.hip -- surrogate-gradient training kernels and the prosody-modulated GIF loop
// (SURVEY.md section 8f-4), fp32 and bf16, channel-contiguous layout [rows][T][H].
//
//   GIF   forward (training): the loop of gif_neuron.py:54-69 that also saves, per step, the
//         pre-clamp potential a_t and the threshold theta_{t-1} it was computed with;
//   GIF   backward: BPTT through T steps with MultiBitSurrogate's triangular window
//         (gif_neuron.py:16-22), the tensor-bound clamp (gradient reaches theta through the
//         bounds when a value is clamped) and the threshold adaptation recurrence;
//   LIF   forward (one step saving the surrogate input; in bf16 also the T-step loop), and backward with
//         LearnableSurrogateGradient (neuron.py:80-108): fast-sigmoid window + slope gradient;
//   ProsodyModulatedGIF forward (prosody_gif.py:69-106): per-(row, t) attention gains scale the
//         input, the effective threshold and the adaptation rate; and its backward.
// One lane owns VEC adjacent channels; state lives in registers over the whole T loop; HBM-bound.
//
// Every kernel exists once, templated on an element policy E (F32 / Bf16 below): the storage type, and r(), the
// rounding each FORWARD op's fp32 result gets -- none in fp32; to bf16, nearest even, under bf16 / autocast, where the
// reference's every op rounds (Python scalars enter as fp32 and are never rounded).  Forward kernels therefore give
// the reference's bits in both dtypes.  A backward kernel recomputes the forward intermediates of a step from the
// saved (a_t, theta_{t-1}) with the same helper the forward uses, roundings included, so the surrogate window and the
// clamp branches are the reference's; its BPTT chain is plain fp32 in both dtypes, gradients stay in fp32 registers
// across the T steps and are rounded once, by the store.  (The reference's bf16 autograd rounds every intermediate
// gradient instead: its result scatters around this one by a few bf16 ulps per step; tests/test_gpu_training.py
// compares both.)  The quotients are true divisions followed by r(), not GifModel's v * rcp(t).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/aura_hip.h"
#include "aura_common.inl"

#pragma clang fp contract(off)

namespace {

#include "aura_gif_model.inl"            // round_bf16
#include "aura_io.inl"                   // Io<T, VEC>, all_aligned16, rtc_grid

struct F32 {
    typedef float T;
    static constexpr bool BF16 = false;
    static constexpr int VEC = 4;        // elements per 16-byte access
    template <int N> using io = Io<float, N>;
    __device__ __forceinline__ static float r(float x) { return x; }
};
struct Bf16 {
    typedef uint16_t T;                  // bit patterns
    static constexpr bool BF16 = true;
    static constexpr int VEC = 8;
    // the element store takes the convert's own 16 bits, one instruction less than Io<uint16_t, 1>'s shift of the
    // rounded float: the scalar instances' instruction text as it was measured (gif_prosody_run went 1.3 % slower
    // with the shift, against a spread of 0.8 %)
    struct Io1 : Io<uint16_t, 1> {
        __device__ __forceinline__ static void store(uint16_t* p, const float (&x)[1]) {
            *p = static_cast<uint16_t>(float_to_bf16_bits(x[0]));
        }
    };
    template <int N> using io = std::conditional_t<N == 1, Io1, Io<uint16_t, N>>;
    __device__ __forceinline__ static float r(float x) { return round_bf16(x); }
};

struct GifP { float decay, Lf, alpha, thr0; };

// forward intermediates of one GIF step from (a, theta_prev): the clamp bound, the clamped potential, the divisor,
// the quotient and the spike count
template <class E>
__device__ __forceinline__ void gif_mid(const GifP& p, float a, float thp, float& cl, float& b, float& d, float& n,
                                        float& s) {
    cl = E::r(E::r(p.Lf * thp) * 2.0f);
    b = fminf(fmaxf(a, -cl), cl);
    d = E::r(thp + 1e-6f);
    n = E::r(b / d);
    s = fminf(fmaxf(floorf(n), 0.0f), p.Lf);
}

template <class E, int VEC>
__global__ __launch_bounds__(256) void gif_fwd_kernel(GifP p, const typename E::T* __restrict__ h,
                                                      typename E::T* __restrict__ spikes, typename E::T* v_io,
                                                      typename E::T* th_io, typename E::T* __restrict__ save_a,
                                                      typename E::T* __restrict__ save_th, int64_t R, int64_t T,
                                                      int64_t C) {
    typedef typename E::template io<VEC> io;
    const int64_t cv = C / VEC, items = R * cv;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items;
         it += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = it / cv, c0 = (it - row * cv) * VEC;
        float v[VEC], th[VEC];
        io::load(v_io + row * C + c0, v);
        io::load(th_io + row * C + c0, th);
        for (int64_t t = 0; t < T; ++t) {
            const int64_t o = (row * T + t) * C + c0;
            float x[VEC], a[VEC], s[VEC], thp[VEC];
            io::load(h + o, x);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                thp[e] = th[e];
                a[e] = E::r(E::r(v[e] * p.decay) + x[e]);
                float cl, b, d, n;
                gif_mid<E>(p, a[e], th[e], cl, b, d, n, s[e]);
                v[e] = E::r(b - E::r(s[e] * th[e]));
                if (p.alpha > 0.0f)
                    th[e] = E::r(E::r(th[e] + E::r(p.alpha * s[e])) - E::r(p.alpha * E::r(th[e] - p.thr0)));
            }
            io::store(spikes + o, s);
            io::store(save_a + o, a);
            io::store(save_th + o, thp);
        }
        io::store(v_io + row * C + c0, v);
        io::store(th_io + row * C + c0, th);
    }
}

// gv_io / gth_io: in = dL/dv_T, dL/dtheta_T; out = dL/dv_0, dL/dtheta_0
template <class E, int VEC>
__global__ __launch_bounds__(256) void gif_bwd_kernel(GifP p, const typename E::T* __restrict__ save_a,
                                                      const typename E::T* __restrict__ save_th,
                                                      const typename E::T* __restrict__ g_spikes,
                                                      typename E::T* __restrict__ g_h, typename E::T* gv_io,
                                                      typename E::T* gth_io, int64_t R, int64_t T, int64_t C) {
    typedef typename E::template io<VEC> io;
    const int64_t cv = C / VEC, items = R * cv;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items;
         it += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = it / cv, c0 = (it - row * cv) * VEC;
        float gv[VEC], gth[VEC];
        io::load(gv_io + row * C + c0, gv);
        io::load(gth_io + row * C + c0, gth);
        for (int64_t t = T - 1; t >= 0; --t) {
            const int64_t o = (row * T + t) * C + c0;
            float a[VEC], thp[VEC], gs[VEC], gh[VEC];
            io::load(save_a + o, a);
            io::load(save_th + o, thp);
            io::load(g_spikes + o, gs);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                float cl, b, d, n, s;
                gif_mid<E>(p, a[e], thp[e], cl, b, d, n, s);
                float gth_prev = gth[e];
                float gs_tot = gs[e];
                if (p.alpha > 0.0f) {            // theta_t = (thp + alpha*s) - alpha*(thp - thr0)
                    gs_tot = gs_tot + p.alpha * gth[e];
                    gth_prev = gth_prev - p.alpha * gth[e];
                }
                gs_tot = gs_tot - thp[e] * gv[e];   // v_t = b - s*thp
                gth_prev = gth_prev - s * gv[e];
                float gb = gv[e];
                const float dist = fabsf(n - rintf(n));
                const float tri = fminf(fmaxf(1.0f - 2.0f * dist, 0.0f), 1.0f);
                const float sur = (n >= 0.0f && n <= p.Lf + 1.0f) ? tri : 0.0f;
                const float gn = gs_tot * sur;
                gb = gb + gn / d;
                gth_prev = gth_prev + (-gn * b / (d * d));
                float ga = 0.0f, gcl = 0.0f;
                if (a[e] < -cl) gcl = -gb;
                else if (a[e] > cl) gcl = gb;
                else ga = gb;
                gth_prev = gth_prev + gcl * (2.0f * p.Lf);
                gh[e] = ga;
                gv[e] = ga * p.decay;
                gth[e] = gth_prev;
            }
            io::store(g_h + o, gh);
        }
        io::store(gv_io + row * C + c0, gv);
        io::store(gth_io + row * C + c0, gth);
    }
}

// ---- LIF (VectorizedLIFNeuron, neuron.py:135-139): mm = r(r(beta m) + x); pre = r(mm - thr); s = pre > 0;
// m' = r(mm - s thr).  TRAIN: the one recording step, which also saves pre; else the T-step loop (bf16 only: the
// fp32 loop is seq_rtc_kernel<LifModel> of aura_neuron.hip).  mem_in may be mem_out.
template <class E, int VEC, bool TRAIN>
__global__ __launch_bounds__(256) void lif_fwd_kernel(const typename E::T* __restrict__ x, const typename E::T* mem_in,
                                                      const typename E::T* __restrict__ beta,
                                                      const typename E::T* __restrict__ thr,
                                                      typename E::T* __restrict__ spk, typename E::T* mem_out,
                                                      typename E::T* __restrict__ pre, int64_t B, int64_t T,
                                                      int64_t C) {
    typedef typename E::template io<VEC> io;
    const int64_t cv = C / VEC, items = B * cv, Tn = TRAIN ? 1 : T;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items;
         it += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = it / cv, c0 = (it - row * cv) * VEC;
        float m[VEC], bt[VEC], th[VEC];
        io::load(mem_in + row * C + c0, m);
        io::load(beta + c0, bt);
        io::load(thr + c0, th);
        for (int64_t t = 0; t < Tn; ++t) {
            const int64_t o = (row * Tn + t) * C + c0;
            float xv[VEC], s[VEC], pr[VEC];
            io::load(x + o, xv);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const float mm = E::r(E::r(bt[e] * m[e]) + xv[e]);
                pr[e] = E::r(mm - th[e]);
                s[e] = pr[e] > 0.0f ? 1.0f : 0.0f;
                m[e] = E::r(mm - s[e] * th[e]);
            }
            io::store(spk + o, s);
            if (TRAIN) io::store(pre + o, pr);
        }
        io::store(mem_out + row * C + c0, m);
    }
}

// g_in = (g_mem_out + (g_spk - g_mem_out*thr) * slope/(|slope*pre|+1)^2); g_x = g_in;
// g_mem_prev = beta * g_in; raw_slope = -(g_spk - g_mem_out*thr) * |pre|*sign(pre)/(slope*|pre|+1)^2
// raw_slope is fp32 in both dtypes: one 16-byte store in fp32, element stores (no alignment asked) in bf16
template <class E, int VEC>
__global__ __launch_bounds__(256) void lif_bwd_kernel(const typename E::T* __restrict__ pre,
                                                      const typename E::T* __restrict__ g_spk,
                                                      const typename E::T* __restrict__ g_mem,
                                                      const typename E::T* __restrict__ beta,
                                                      const typename E::T* __restrict__ thr,
                                                      const typename E::T* __restrict__ slope,
                                                      typename E::T* __restrict__ g_x,
                                                      typename E::T* __restrict__ g_mem_prev,
                                                      float* __restrict__ raw_slope, int64_t B, int64_t C) {
    typedef typename E::template io<VEC> io;
    const int64_t cv = C / VEC, items = B * cv;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items;
         it += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = it / cv, c0 = (it - row * cv) * VEC;
        float pr[VEC], gs[VEC], gm[VEC], bt[VEC], th[VEC], sl[VEC], gx[VEC], gp[VEC], rs[VEC];
        io::load(pre + row * C + c0, pr);
        io::load(g_spk + row * C + c0, gs);
        io::load(g_mem + row * C + c0, gm);
        io::load(beta + c0, bt);
        io::load(thr + c0, th);
        io::load(slope + c0, sl);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float g_s = gs[e] - gm[e] * th[e];         // spk feeds the output and mem_out = mem - spk*thr
            const float den = fabsf(sl[e] * pr[e]) + 1.0f;
            const float g_pre = g_s * (sl[e] / (den * den));
            const float g_m = gm[e] + g_pre;                 // grad of mem' = beta*mem + x
            gx[e] = g_m;
            gp[e] = bt[e] * g_m;
            const float ap = fabsf(pr[e]);
            const float sg = pr[e] > 0.0f ? 1.0f : (pr[e] < 0.0f ? -1.0f : 0.0f);
            const float den2 = sl[e] * ap + 1.0f;
            rs[e] = -g_s * ap * sg / (den2 * den2);
            if (E::BF16) raw_slope[row * C + c0 + e] = rs[e];
        }
        io::store(g_x + row * C + c0, gx);
        io::store(g_mem_prev + row * C + c0, gp);
        if constexpr (!E::BF16) Io<float, VEC>::store(raw_slope + row * C + c0, rs);
    }
}

// ---- ProsodyModulatedGIF (prosody_gif.py:64-106; under .bfloat16() x, state AND gains are bf16) ---------------------
// The per (row, t) quantities are rounded chains too: scale = clamp(r(1 - r(str * r(g - 1))), .5, 1.5),
// ae = r(alpha g); live: torch.clamp passes the gradient at the bounds.  No gains: no modulation.
struct ProsodyStep { float g, scale, ae; bool live; };
template <class E>
__device__ __forceinline__ ProsodyStep prosody_step(const GifP& p, float strength, const typename E::T* gains, int64_t at) {
    ProsodyStep r;
    if (gains == nullptr) { r.g = 1.0f; r.scale = 1.0f; r.ae = p.alpha; r.live = false; return r; }
    float g[1];
    Io<typename E::T, 1>::load(gains + at, g);
    r.g = g[0];
    const float raw = E::r(1.0f - E::r(strength * E::r(r.g - 1.0f)));
    r.scale = fminf(fmaxf(raw, 0.5f), 1.5f);
    r.live = raw >= 0.5f && raw <= 1.5f;
    r.ae = E::r(p.alpha * r.g);
    return r;
}
// forward intermediates of one step from (a, theta_prev): te, cl, b, n, s; no 1e-6 in the division (unlike GIFNeuron)
template <class E>
__device__ __forceinline__ void prosody_mid(const GifP& p, bool mod, float scale, float a, float thp, float& te,
                                            float& cl, float& b, float& n, float& s) {
    te = mod ? E::r(thp * scale) : thp;
    cl = E::r(E::r(p.Lf * te) * 2.0f);
    b = fminf(fmaxf(a, -cl), cl);
    n = E::r(b / te);
    s = fminf(fmaxf(floorf(n), 0.0f), p.Lf);
}

// SAVE = the recording forward: also the pre-clamp potential a_t and the threshold theta_{t-1} of every step
// (everything else is recomputed in backward)
template <class E, int VEC, bool SAVE>
__global__ __launch_bounds__(256) void prosody_fwd_kernel(GifP p, float strength, const typename E::T* __restrict__ h,
                                                          const typename E::T* __restrict__ gains,
                                                          typename E::T* __restrict__ spikes, typename E::T* v_io,
                                                          typename E::T* th_io, typename E::T* __restrict__ save_a,
                                                          typename E::T* __restrict__ save_th, int64_t R, int64_t T,
                                                          int64_t C) {
    typedef typename E::template io<VEC> io;
    const int64_t cv = C / VEC, items = R * cv;
    const bool mod = gains != nullptr;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items;
         it += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = it / cv, c0 = (it - row * cv) * VEC;
        float v[VEC], th[VEC];
        io::load(v_io + row * C + c0, v);
        io::load(th_io + row * C + c0, th);
        for (int64_t t = 0; t < T; ++t) {
            const int64_t o = (row * T + t) * C + c0;
            float x[VEC], a[VEC], s[VEC], thp[VEC];
            io::load(h + o, x);
            const ProsodyStep ps = prosody_step<E>(p, strength, gains, row * T + t);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                thp[e] = th[e];
                const float i_t = mod ? E::r(x[e] * ps.g) : x[e];
                a[e] = E::r(E::r(v[e] * p.decay) + i_t);
                float te, cl, b, n;
                prosody_mid<E>(p, mod, ps.scale, a[e], th[e], te, cl, b, n, s[e]);
                v[e] = E::r(b - E::r(s[e] * te));
                if (p.alpha > 0.0f)
                    th[e] = E::r(E::r(th[e] + E::r(ps.ae * s[e])) - E::r(ps.ae * E::r(th[e] - p.thr0)));
            }
            io::store(spikes + o, s);
            if (SAVE) { io::store(save_a + o, a); io::store(save_th + o, thp); }
        }
        io::store(v_io + row * C + c0, v);
        io::store(th_io + row * C + c0, th);
    }
}

// Backward of that loop (BPTT, reverse time).  Per step, with g = gains[row][t], scale = clamp(1 - str (g - 1),
// 0.5, 1.5), te = thp scale, ae = alpha g:
//   theta_t = thp + ae s - ae (thp - thr0);  v_t = b - s te;  s = surrogate(n), n = b / te;
//   b = clamp(a, -2 L te, 2 L te);  a = v_{t-1} decay + x g.
// Besides dL/dh and the initial-state gradients it returns dL/dgains[row][t] (fp32 in both dtypes, summed over the
// channels with float atomics: g_gains must be zeroed by the caller): through the input gain (x), the threshold scale
// (-strength where the clamp is inactive) and the adaptation rate (alpha).
template <class E, int VEC>
__global__ __launch_bounds__(256) void prosody_bwd_kernel(GifP p, float strength,
                                                          const typename E::T* __restrict__ save_a,
                                                          const typename E::T* __restrict__ save_th,
                                                          const typename E::T* __restrict__ h,
                                                          const typename E::T* __restrict__ gains,
                                                          const typename E::T* __restrict__ g_spikes,
                                                          typename E::T* __restrict__ g_h, float* __restrict__ g_gains,
                                                          typename E::T* gv_io, typename E::T* gth_io, int64_t R,
                                                          int64_t T, int64_t C) {
    typedef typename E::template io<VEC> io;
    const int64_t cv = C / VEC, items = R * cv;
    const bool mod = gains != nullptr;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items;
         it += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = it / cv, c0 = (it - row * cv) * VEC;
        float gv[VEC], gth[VEC];
        io::load(gv_io + row * C + c0, gv);
        io::load(gth_io + row * C + c0, gth);
        for (int64_t t = T - 1; t >= 0; --t) {
            const int64_t o = (row * T + t) * C + c0;
            float a[VEC], thp[VEC], gs[VEC], gh[VEC], x[VEC];
            io::load(save_a + o, a);
            io::load(save_th + o, thp);
            io::load(g_spikes + o, gs);
            io::load(h + o, x);
            const ProsodyStep ps = prosody_step<E>(p, strength, gains, row * T + t);
            float gg = 0.0f;                                             // this lane's share of dL/dgains[row][t]
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                float te, cl, b, n, s;
                prosody_mid<E>(p, mod, ps.scale, a[e], thp[e], te, cl, b, n, s);
                float gth_prev = gth[e];
                float gs_tot = gs[e];
                if (p.alpha > 0.0f) {
                    gs_tot = gs_tot + ps.ae * gth[e];
                    gth_prev = gth_prev - ps.ae * gth[e];
                    if (mod) gg += gth[e] * (s - (thp[e] - p.thr0)) * p.alpha;
                }
                gs_tot = gs_tot - te * gv[e];                            // v_t = b - s te
                float gte = -s * gv[e];
                float gb = gv[e];
                const float dist = fabsf(n - rintf(n));
                const float tri = fminf(fmaxf(1.0f - 2.0f * dist, 0.0f), 1.0f);
                const float sur = (n >= 0.0f && n <= p.Lf + 1.0f) ? tri : 0.0f;
                const float gn = gs_tot * sur;
                gb = gb + gn / te;
                gte = gte + (-gn * b / (te * te));
                float ga = 0.0f, gcl = 0.0f;
                if (a[e] < -cl) gcl = -gb;
                else if (a[e] > cl) gcl = gb;
                else ga = gb;
                gte = gte + gcl * (2.0f * p.Lf);
                gth_prev = gth_prev + (mod ? gte * ps.scale : gte);
                if (ps.live) gg += gte * thp[e] * (-strength);
                gh[e] = mod ? ga * ps.g : ga;
                if (mod) gg += ga * x[e];
                gv[e] = ga * p.decay;
                gth[e] = gth_prev;
            }
            io::store(g_h + o, gh);
            if (mod && g_gains) atomicAdd(g_gains + row * T + t, gg);
        }
        io::store(gv_io + row * C + c0, gv);
        io::store(gth_io + row * C + c0, gth);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------
template <class E> const typename E::T* rd(const void* p) { return static_cast<const typename E::T*>(p); }
template <class E> typename E::T* wr(void* p) { return static_cast<typename E::T*>(p); }

template <class T> struct as_is { typedef T type; };

// The one launch form: rows x C channels through the 16-byte instance kv (vec channels per work item) when C divides
// and every tensor named in `aligned` allows it, else through the scalar instance k1.  The arguments convert to the
// kernel's own parameter types.
template <class... KA>
int launch_rows(void (*kv)(KA...), void (*k1)(KA...), int vec, bool aligned, int64_t rows, int64_t C, hipStream_t s,
                typename as_is<KA>::type... args) {
    const bool wide = C % vec == 0 && aligned;
    void* argv[] = {&args...};
    (void)hipLaunchKernel(reinterpret_cast<const void*>(wide ? kv : k1),
                          dim3(rtc_grid(wide ? rows * (C / vec) : rows * C)), dim3(256), argv, 0, s);
    return aura_check_launch();
}

// spike counts up to 256 are exact in bf16
template <class E> bool bad_gif_sizes(int64_t rows, int64_t T, int64_t H, int L) {
    return rows < 0 || T < 0 || H < 0 || L < 0 || (E::BF16 && L > 256);
}

template <class E>
int gif_train_forward(const void* h, void* spikes, void* v, void* theta, void* save_a, void* save_theta, float decay,
                      int L, float alpha, float threshold, int64_t rows, int64_t T, int64_t H, hipStream_t s) {
    if (bad_gif_sizes<E>(rows, T, H, L)) return AURA_E_INVAL;
    if (rows == 0 || H == 0) return AURA_OK;
    if (!v || !theta || (T && (!h || !spikes || !save_a || !save_theta))) return AURA_E_INVAL;
    return launch_rows(gif_fwd_kernel<E, E::VEC>, gif_fwd_kernel<E, 1>, E::VEC,
                       all_aligned16(h, spikes, v, theta, save_a, save_theta), rows, H, s,
                       GifP{decay, (float)L, alpha, threshold}, rd<E>(h), wr<E>(spikes), wr<E>(v), wr<E>(theta),
                       wr<E>(save_a), wr<E>(save_theta), rows, T, H);
}

template <class E>
int gif_backward(const void* save_a, const void* save_theta, const void* g_spikes, void* g_h, void* g_v, void* g_theta,
                 float decay, int L, float alpha, float threshold, int64_t rows, int64_t T, int64_t H, hipStream_t s) {
    if (bad_gif_sizes<E>(rows, T, H, L)) return AURA_E_INVAL;
    if (rows == 0 || H == 0) return AURA_OK;
    if (!g_v || !g_theta || (T && (!save_a || !save_theta || !g_spikes || !g_h))) return AURA_E_INVAL;
    return launch_rows(gif_bwd_kernel<E, E::VEC>, gif_bwd_kernel<E, 1>, E::VEC,
                       all_aligned16(save_a, save_theta, g_spikes, g_h, g_v, g_theta), rows, H, s,
                       GifP{decay, (float)L, alpha, threshold}, rd<E>(save_a), rd<E>(save_theta), rd<E>(g_spikes),
                       wr<E>(g_h), wr<E>(g_v), wr<E>(g_theta), rows, T, H);
}

template <class E>
int lif_train_forward(const void* x, const void* mem_in, const void* beta, const void* threshold, void* spikes,
                      void* mem_out, void* pre, int64_t B, int64_t size, hipStream_t s) {
    if (B < 0 || size < 0) return AURA_E_INVAL;
    if (B == 0 || size == 0) return AURA_OK;
    if (!x || !mem_in || !beta || !threshold || !spikes || !mem_out || !pre) return AURA_E_INVAL;
    return launch_rows(lif_fwd_kernel<E, E::VEC, true>, lif_fwd_kernel<E, 1, true>, E::VEC,
                       all_aligned16(x, mem_in, beta, threshold, spikes, mem_out, pre), B, size, s, rd<E>(x),
                       rd<E>(mem_in), rd<E>(beta), rd<E>(threshold), wr<E>(spikes), wr<E>(mem_out), wr<E>(pre), B, 1,
                       size);
}

template <class E>
int lif_backward(const void* pre, const void* g_spikes, const void* g_mem, const void* beta, const void* threshold,
                 const void* slope, void* g_x, void* g_mem_prev, float* raw_slope, int64_t B, int64_t size,
                 hipStream_t s) {
    if (B < 0 || size < 0) return AURA_E_INVAL;
    if (B == 0 || size == 0) return AURA_OK;
    if (!pre || !g_spikes || !g_mem || !beta || !threshold || !slope || !g_x || !g_mem_prev || !raw_slope)
        return AURA_E_INVAL;
    return launch_rows(lif_bwd_kernel<E, E::VEC>, lif_bwd_kernel<E, 1>, E::VEC,
                       all_aligned16(pre, g_spikes, g_mem, beta, threshold, slope, g_x, g_mem_prev) &&
                           (E::BF16 || aligned16(raw_slope)),
                       B, size, s, rd<E>(pre), rd<E>(g_spikes), rd<E>(g_mem), rd<E>(beta), rd<E>(threshold),
                       rd<E>(slope), wr<E>(g_x), wr<E>(g_mem_prev), raw_slope, B, size);
}

// save_a == NULL and save_theta == NULL: the plain loop (aura_gif_prosody_run)
template <class E, bool SAVE>
int gif_prosody_forward(const void* h, const void* gains, void* spikes, void* v, void* theta, void* save_a,
                        void* save_theta, float decay, int L, float alpha, float threshold, float strength,
                        int64_t rows, int64_t T, int64_t H, hipStream_t s) {
    if (bad_gif_sizes<E>(rows, T, H, L)) return AURA_E_INVAL;
    if (rows == 0 || H == 0) return AURA_OK;
    if (!v || !theta || (T && (!h || !spikes || (SAVE && (!save_a || !save_theta))))) return AURA_E_INVAL;
    return launch_rows(prosody_fwd_kernel<E, E::VEC, SAVE>, prosody_fwd_kernel<E, 1, SAVE>, E::VEC,
                       all_aligned16(h, spikes, v, theta, save_a, save_theta), rows, H, s,
                       GifP{decay, (float)L, alpha, threshold}, strength, rd<E>(h), rd<E>(gains), wr<E>(spikes),
                       wr<E>(v), wr<E>(theta), wr<E>(save_a), wr<E>(save_theta), rows, T, H);
}

template <class E>
int gif_prosody_backward(const void* save_a, const void* save_theta, const void* h, const void* gains,
                         const void* g_spikes, void* g_h, float* g_gains, void* g_v, void* g_theta, float decay, int L,
                         float alpha, float threshold, float strength, int64_t rows, int64_t T, int64_t H,
                         hipStream_t s) {
    if (bad_gif_sizes<E>(rows, T, H, L)) return AURA_E_INVAL;
    if (rows == 0 || H == 0) return AURA_OK;
    if (!g_v || !g_theta || (T && (!save_a || !save_theta || !h || !g_spikes || !g_h))) return AURA_E_INVAL;
    return launch_rows(prosody_bwd_kernel<E, E::VEC>, prosody_bwd_kernel<E, 1>, E::VEC,
                       all_aligned16(save_a, save_theta, h, g_spikes, g_h, g_v, g_theta), rows, H, s,
                       GifP{decay, (float)L, alpha, threshold}, strength, rd<E>(save_a), rd<E>(save_theta), rd<E>(h),
                       rd<E>(gains), rd<E>(g_spikes), wr<E>(g_h), g_gains, wr<E>(g_v), wr<E>(g_theta), rows, T, H);
}

}  // namespace

// aura_lif_run's bf16 form (the entry point is in aura_neuron.hip, beside the fp32 loop); internal to the library
__attribute__((visibility("hidden"))) int aura_lif_seq_bf16(const uint16_t* x, uint16_t* spikes, uint16_t* mem,
                                                            const uint16_t* beta, const uint16_t* threshold, int64_t B,
                                                            int64_t T, int64_t size, hipStream_t stream) {
    if (B < 0 || T < 0 || size < 0) return AURA_E_INVAL;
    if (B == 0 || size == 0 || T == 0) return AURA_OK;
    if (!x || !spikes || !mem || !beta || !threshold) return AURA_E_INVAL;
    return launch_rows(lif_fwd_kernel<Bf16, 8, false>, lif_fwd_kernel<Bf16, 1, false>, 8,
                       all_aligned16(x, spikes, mem, beta, threshold), B, size, stream, x, mem, beta, threshold, spikes,
                       mem, nullptr, B, T, size);
}

// the call, which names the element policy E, for the dtype code; any other code is refused before anything is launched
#define AURA_BY_DTYPE(...)                                                            \
    (dtype == AURA_DTYPE_F32    ? [&] { using E = F32; return __VA_ARGS__; }()        \
     : dtype == AURA_DTYPE_BF16 ? [&] { using E = Bf16; return __VA_ARGS__; }()       \
                                : AURA_E_INVAL)

extern "C" {

int aura_gif_train_forward(const void* h, void* spikes, void* v, void* theta, void* save_a, void* save_theta,
                           float decay, int L, float alpha, float threshold, int64_t rows, int64_t T, int64_t H,
                           int dtype, void* stream) {
    return AURA_BY_DTYPE(gif_train_forward<E>(h, spikes, v, theta, save_a, save_theta, decay, L, alpha, threshold, rows,
                         T, H, static_cast<hipStream_t>(stream)));
}

int aura_gif_backward(const void* save_a, const void* save_theta, const void* g_spikes, void* g_h, void* g_v,
                      void* g_theta, float decay, int L, float alpha, float threshold, int64_t rows, int64_t T,
                      int64_t H, int dtype, void* stream) {
    return AURA_BY_DTYPE(gif_backward<E>(save_a, save_theta, g_spikes, g_h, g_v, g_theta, decay, L, alpha, threshold,
                         rows, T, H, static_cast<hipStream_t>(stream)));
}

int aura_lif_train_forward(const void* x, const void* mem_in, const void* beta, const void* threshold, void* spikes,
                           void* mem_out, void* pre, int64_t B, int64_t size, int dtype, void* stream) {
    return AURA_BY_DTYPE(lif_train_forward<E>(x, mem_in, beta, threshold, spikes, mem_out, pre, B, size,
                         static_cast<hipStream_t>(stream)));
}

int aura_lif_backward(const void* pre, const void* g_spikes, const void* g_mem, const void* beta,
                      const void* threshold, const void* slope, void* g_x, void* g_mem_prev, float* raw_slope,
                      int64_t B, int64_t size, int dtype, void* stream) {
    return AURA_BY_DTYPE(lif_backward<E>(pre, g_spikes, g_mem, beta, threshold, slope, g_x, g_mem_prev, raw_slope, B,
                         size, static_cast<hipStream_t>(stream)));
}

int aura_gif_prosody_run(const void* h, const void* gains, void* spikes, void* v, void* theta, float decay, int L,
                         float alpha, float threshold, float strength, int64_t rows, int64_t T, int64_t H, int dtype,
                         void* stream) {
    return AURA_BY_DTYPE(gif_prosody_forward<E, false>(h, gains, spikes, v, theta, nullptr, nullptr, decay, L, alpha,
                          threshold, strength, rows, T, H, static_cast<hipStream_t>(stream)));
}

int aura_gif_prosody_train_forward(const void* h, const void* gains, void* spikes, void* v, void* theta, void* save_a,
                                   void* save_theta, float decay, int L, float alpha, float threshold, float strength,
                                   int64_t rows, int64_t T, int64_t H, int dtype, void* stream) {
    return AURA_BY_DTYPE(gif_prosody_forward<E, true>(h, gains, spikes, v, theta, save_a, save_theta, decay, L, alpha,
                          threshold, strength, rows, T, H, static_cast<hipStream_t>(stream)));
}

int aura_gif_prosody_backward(const void* save_a, const void* save_theta, const void* h, const void* gains,
                              const void* g_spikes, void* g_h, float* g_gains, void* g_v, void* g_theta, float decay,
                              int L, float alpha, float threshold, float strength, int64_t rows, int64_t T, int64_t H,
                              int dtype, void* stream) {
    return AURA_BY_DTYPE(gif_prosody_backward<E>(save_a, save_theta, h, gains, g_spikes, g_h, g_gains, g_v, g_theta,
                         decay, L, alpha, threshold, strength, rows, T, H, static_cast<hipStream_t>(stream)));
}

}  // extern "C"
