// aura_retention.inl -- the retention key and its order, shared by the selections of aura_bank.hip and aura_quota.hip
// (one definition: the two must rank a row alike to the last bit).  Included inside each file's anonymous namespace;
// needs aura_common.inl.
//   key(r) = strength(r) * aura_recency(now, timestamp(r))        -- expf(-(now - timestamp) / 3600)
//   comp(r) = ordered_u32(key(r)) << 32 | (r - origin) mod count      -- ascending comp = the eviction order

__device__ __forceinline__ float retention_key(float strength, float timestamp, float now) {
    return strength * aura_recency(now, timestamp);
}

// order-preserving map fp32 -> u32: NaN lowest (0), then -inf .. -0 == +0 .. +inf
__device__ __forceinline__ uint32_t retention_ordered(float key) {
    if (key != key) return 0u;
    if (key == 0.0f) return 0x80000000u;
    const uint32_t u = __float_as_uint(key);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ uint64_t retention_comp(uint32_t okey, int64_t r, int64_t cursor, int64_t count) {
    int64_t rot = r - cursor;
    if (rot < 0) rot += count;
    return ((uint64_t)okey << 32) | (uint64_t)rot;
}
