// aura_io.inl -- element I/O and launch geometry of the channel-contiguous neuron kernels, shared by aura_neuron.hip
// and aura_train.hip: Io<T, VEC> moves VEC adjacent channels (fp32, or bf16 bit patterns widened to fp32 registers)
// with one 16-byte access, and the host side decides whether a call may use it.  Included inside the including file's
// anonymous namespace, after aura_gif_model.inl (round_bf16).

// ------------------------------------------------------------------------------------------
// 16-byte vector I/O
// ------------------------------------------------------------------------------------------
template <typename T, int VEC>
struct Io;

template <>
struct Io<float, 4> {
    __device__ __forceinline__ static void load(const float* p, float (&x)[4]) {
        float4 t = *reinterpret_cast<const float4*>(p);
        x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
    }
    __device__ __forceinline__ static void store(float* p, const float (&x)[4]) {
        *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
    }
    // streaming (touched once) tensors: non-temporal, so they do not evict each other from L2
    typedef float v4f __attribute__((ext_vector_type(4)));
    __device__ __forceinline__ static void load_nt(const float* p, float (&x)[4]) {
        const v4f t = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(p));
        x[0] = t[0]; x[1] = t[1]; x[2] = t[2]; x[3] = t[3];
    }
    __device__ __forceinline__ static void store_nt(float* p, const float (&x)[4]) {
        const v4f t = {x[0], x[1], x[2], x[3]};
        __builtin_nontemporal_store(t, reinterpret_cast<v4f*>(p));
    }
};
template <>
struct Io<float, 1> {
    __device__ __forceinline__ static void load(const float* p, float (&x)[1]) { x[0] = *p; }
    __device__ __forceinline__ static void store(float* p, const float (&x)[1]) { *p = x[0]; }
    __device__ __forceinline__ static void load_nt(const float* p, float (&x)[1]) { x[0] = __builtin_nontemporal_load(p); }
    __device__ __forceinline__ static void store_nt(float* p, const float (&x)[1]) { __builtin_nontemporal_store(x[0], p); }
};

__device__ __forceinline__ float bf16_bits_to_float(uint32_t b) { return __uint_as_float(b << 16); }
// round to nearest even; the 16-byte store packs the convert's own 16 bits, the element store shifts the rounded
// float down: the same bits, each in the form the instruction text of its kernels was measured with
__device__ __forceinline__ uint32_t float_to_bf16_bits(float x) {
    return __builtin_bit_cast(uint16_t, static_cast<__bf16>(x));
}

template <>
struct Io<uint16_t, 8> {
    __device__ __forceinline__ static void load(const uint16_t* p, float (&x)[8]) {
        uint4 t = *reinterpret_cast<const uint4*>(p);
        uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x[2 * i] = __uint_as_float(w[i] << 16);
            x[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
        }
    }
    __device__ __forceinline__ static void store(uint16_t* p, const float (&x)[8]) {
        uint32_t w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            w[i] = float_to_bf16_bits(x[2 * i]) | (float_to_bf16_bits(x[2 * i + 1]) << 16);
        *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    // bf16 streams keep the default cache policy: non-temporal measured slower here (the bf16 GIF
    // loop is VALU-bound: 0.67 vs 0.54 ms at 8192 x 16 x 3072), while it took the fp32 GIF loop from
    // 5.5 to 6.4 TB/s
    __device__ __forceinline__ static void load_nt(const uint16_t* p, float (&x)[8]) { load(p, x); }
    __device__ __forceinline__ static void store_nt(uint16_t* p, const float (&x)[8]) { store(p, x); }
};
template <>
struct Io<uint16_t, 1> {
    __device__ __forceinline__ static void load_nt(const uint16_t* p, float (&x)[1]) { load(p, x); }
    __device__ __forceinline__ static void store_nt(uint16_t* p, const float (&x)[1]) { store(p, x); }
    __device__ __forceinline__ static void load(const uint16_t* p, float (&x)[1]) {
        x[0] = bf16_bits_to_float(*p);
    }
    __device__ __forceinline__ static void store(uint16_t* p, const float (&x)[1]) {
        *p = static_cast<uint16_t>(__float_as_uint(round_bf16(x[0])) >> 16);
    }
};

// ------------------------------------------------------------------------------------------
// Host side: may a call take the 16-byte path, and how many blocks stream its work items
// ------------------------------------------------------------------------------------------
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
template <class... P>
inline bool all_aligned16(const P*... p) { return (aligned16(p) && ...); }

inline int rtc_grid(int64_t items) {
    // memory-bound streaming: cap at 256 CUs x 8 blocks and grid-stride the rest
    int64_t blocks = (items + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}
