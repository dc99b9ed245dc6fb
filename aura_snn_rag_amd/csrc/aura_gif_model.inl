// aura_gif_model.inl -- the GIF neuron step (and the bf16 rounding helpers it needs), shared by the neuron loops of
// aura_neuron.hip and the GIF epilogue of aura_rowlin.hip: one definition, so that both give the same bits.  Included
// inside the including file's anonymous namespace, after <hip/hip_runtime.h>.

__device__ __forceinline__ float round_bf16(float x) {
    // round-to-nearest-even through the hardware convert (v_cvt_pk_bf16_f32); NaN stays NaN
    return static_cast<float>(static_cast<__bf16>(x));
}

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// two roundings for the price of one convert: v_cvt_pk_bf16_f32 packs both results
__device__ __forceinline__ void round_bf16_pair(float& a, float& b) {
    const f32x2 f = {a, b};
    const f32x2 g = __builtin_convertvector(__builtin_convertvector(f, bf16x2), f32x2);
    a = g.x;
    b = g.y;
}

// src/core/language_zone/gif_neuron.py:56-67.  BF16 = state and every intermediate are bf16
// tensors in the reference, i.e. each op rounds its fp32 result to bf16.
//
// Two exact shortcuts of the bf16 loop (13 roundings per step):
//  * the quotient.  The reference divides two bf16 tensors: RNE_bf16(RN_fp32(v / t)).  v and t carry
//    8-bit significands, so the real quotient x = (mv / mt) 2^e is never a bf16 rounding midpoint
//    (a dyadic mv / mt has at most 8 significant bits) and lies at least 2^-17 (relative) away from
//    every midpoint: |mv 2^s 256 - N mt| >= 1 for odd N, mt <= 255.  Any approximation of x that is
//    good to 2^-18 therefore rounds to the same bf16 value: v * rcp(t) (v_rcp_f32: 1 ulp) replaces
//    the ~10-instruction IEEE division, bit for bit (the whole bf16 GIF suite, and the exhaustive
//    significand-pair proof in the CPU test suite, test_bf16_quotients_are_never_near_a_rounding_midpoint).
//  * POW2L: for L a power of two, L * theta and its doubling are exact in bf16: no rounding.
template <bool BF16, bool POW2L = false>
struct GifModel {
    float decay, Lf, alpha, thr0;
    static constexpr int NS = 2;
    struct Lane { float s0, s1; };
    __device__ __forceinline__ static float r(float x) { return BF16 ? round_bf16(x) : x; }
    __device__ __forceinline__ static void r2(float& a, float& b) { if (BF16) round_bf16_pair(a, b); }
    __device__ __forceinline__ static float quot(float v, float t) {
        return BF16 ? v * __builtin_amdgcn_rcpf(t) : v / t;
    }
    __device__ __forceinline__ void init(Lane&, int64_t) const {}
    // two neurons at once: the same op sequence as step(), roundings paired (bf16 build: 3 VALU
    // ops per two roundings instead of 4).  x*2 of a bf16 value is exact, so r(r(L*theta)*2) is
    // r(L*theta)*2.
    __device__ __forceinline__ void step2(Lane& la, Lane& lb, float ia, float ib, float& sa,
                                          float& sb) const {
        float va = la.s0 * decay, vb = lb.s0 * decay;           r2(va, vb);
        va = va + ia; vb = vb + ib;                               r2(va, vb);
        float ca = Lf * la.s1, cb = Lf * lb.s1;                   if (!POW2L) r2(ca, cb);
        ca = ca * 2.0f; cb = cb * 2.0f;
        va = fminf(fmaxf(va, -ca), ca); vb = fminf(fmaxf(vb, -cb), cb);
        float ta = la.s1 + 1e-6f, tb = lb.s1 + 1e-6f;             r2(ta, tb);
        float na = quot(va, ta), nb = quot(vb, tb);               r2(na, nb);
        sa = fminf(fmaxf(floorf(na), 0.0f), Lf); sb = fminf(fmaxf(floorf(nb), 0.0f), Lf);
        float pa = sa * la.s1, pb = sb * lb.s1;                   r2(pa, pb);
        va = va - pa; vb = vb - pb;                               r2(va, vb);
        float tha = la.s1, thb = lb.s1;
        if (alpha > 0.0f) {
            float ea = alpha * sa, eb = alpha * sb;               r2(ea, eb);
            float ua = tha + ea, ub = thb + eb;                   r2(ua, ub);
            float da = tha - thr0, db = thb - thr0;               r2(da, db);
            da = alpha * da; db = alpha * db;                     r2(da, db);
            tha = ua - da; thb = ub - db;                         r2(tha, thb);
        }
        la.s0 = va; la.s1 = tha;
        lb.s0 = vb; lb.s1 = thb;
    }
    __device__ __forceinline__ float step(Lane& l, float i_t) const {
        float v = l.s0, theta = l.s1;
        v = r(r(v * decay) + i_t);
        float cl = r(r(Lf * theta) * 2.0f);
        v = fminf(fmaxf(v, -cl), cl);
        float nv = r(quot(v, r(theta + 1e-6f)));
        float spike = fminf(fmaxf(floorf(nv), 0.0f), Lf);
        v = r(v - r(spike * theta));
        if (alpha > 0.0f) theta = r(r(theta + r(alpha * spike)) - r(alpha * r(theta - thr0)));
        l.s0 = v;
        l.s1 = theta;
        return spike;
    }
};
