// aura_select.inl -- the radix selection over 64-bit composites  ordered key << 32 | rotated row, shared by the
// retention selection (aura_bank.hip: the n weakest rows) and the replay draw (aura_replay.hip: the n largest draw
// keys, as the n smallest REVERSED ordered keys with cursor 0).  One definition: both take exactly the n smallest
// composites.  Included inside each file's anonymous namespace; needs aura_common.inl and aura_retention.inl.
//   pass 0   the caller's own kernel: reads the metadata once, stores a 32-bit ordered key per row (4 B per row),
//            histograms its top 12 bits (sel_hist_add) and keeps min / max of the ordered keys (sel_minmax_flush)
//   pass i   select_pass_kernel reads the 4-byte ordered keys; every workgroup first narrows the prefix from the
//            previous pass's histogram (the same 4096-bin scan in every workgroup: no launch in between), then
//            histograms the next digit of the rows that match the prefix.  Digits: 12 + 12 + 8 bits of the key, then
//            the bits of the rotated row that `count` needs, 12 at a time (sel_passes).
//   compact  sel_compact writes the rows with comp <= threshold: a workgroup collects its rows in LDS and reserves
//            their output range with ONE global add (4096 single adds to one address cost 44 us).  What is written per
//            row, and which rows take no part whatever their composite, is the caller's (the Out argument).
// Histograms live in LDS; a workgroup adds each non-empty bin to the global histogram once (integer adds: the result
// does not depend on arrival order).  Keys that share their leading bits put every workgroup's adds on the same few
// addresses (a same-address atomic costs ~1.4 ns: 2048 workgroups x 16 bins took 50 us), so the grid is capped at 512
// workgroups and the global histogram is kept in SEL_COPIES copies (workgroup b adds to copy b mod SEL_COPIES; the
// narrowing step sums them).  A pass whose chosen bin holds exactly the rows still needed ends the selection early
// (distinct keys: after the key digits); later launches return at once.  Equal keys are seen by pass 0 (min == max):
// the threshold is then the rotated row n - 1 itself and nothing but pass 0 and the compaction reads the rows.

constexpr int SEL_BINS = 4096;          // 12-bit digits
constexpr int SEL_MAX_PASSES = 6;       // 3 digits of the key + at most 3 of a 31-bit rotated row
constexpr int SEL_MAX_BLOCKS = 512;
constexpr int SEL_COPIES = 4;           // copies of every global histogram
constexpr int SEL_LIST = 2048;          // selected rows a workgroup of the compaction holds before it writes them out

struct SelState {                       // one per pass: written by workgroup 0 of pass i, read by pass i + 1
    unsigned long long prefix;          // decided high bits of the threshold; the threshold itself once done
    uint32_t need;                      // rows still to take among those that match the prefix
    uint32_t done;
    uint32_t kmax, kmin_inv;            // [0] only: max / ~min of the ordered keys (pass 0)
    uint32_t out_count;                 // [0] only: the compaction's cursor
    uint32_t pad;
};

__device__ __forceinline__ void sel_flush_hist(const uint32_t* s_hist, int bins, uint32_t* __restrict__ hist) {
    hist += (blockIdx.x % SEL_COPIES) * SEL_BINS;
    for (int b = threadIdx.x; b < bins; b += 256) {
        const uint32_t c = s_hist[b];
        if (c) atomicAdd(&hist[b], c);
    }
}

__device__ __forceinline__ uint32_t sel_bin(const uint32_t* __restrict__ hist, int b) {
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < SEL_COPIES; ++j) c += hist[j * SEL_BINS + b];
    return c;
}

// pass 0, one row's digit d (the top 12 bits of its ordered key) into the workgroup's histogram: a wave whose lanes
// agree (a bank of equal or nearly equal keys) adds once instead of 64 times to one address
__device__ __forceinline__ void sel_hist_add(uint32_t* s_hist, uint32_t d) {
    const uint32_t d0 = __builtin_amdgcn_readfirstlane(d);
    if (__all(d == d0)) {
        const unsigned long long act = __ballot(1);
        if ((int)__lane_id() == __ffsll(act) - 1) atomicAdd(&s_hist[d0], (uint32_t)__popcll(act));
    } else {
        atomicAdd(&s_hist[d], 1u);
    }
}

// pass 0, the end: the workgroup's histogram and its max / ~min of the ordered keys (s_mm[2], zeroed with the
// histogram) join the global ones
__device__ __forceinline__ void sel_minmax_flush(uint32_t kmax, uint32_t kmin_inv, const uint32_t* s_hist, uint32_t* s_mm,
                                                 uint32_t* __restrict__ hist, SelState* __restrict__ st0) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, off));
        kmin_inv = max(kmin_inv, (uint32_t)__shfl_xor((int)kmin_inv, off));
    }
    if ((threadIdx.x & 63) == 0) { atomicMax(&s_mm[0], kmax); atomicMax(&s_mm[1], kmin_inv); }
    __syncthreads();
    sel_flush_hist(s_hist, SEL_BINS, hist);
    if (threadIdx.x == 0) { atomicMax(&st0->kmax, s_mm[0]); atomicMax(&st0->kmin_inv, s_mm[1]); }
}

// Narrow the threshold with the histogram of the pass before (digit at prev_shift, prev_width bits).  Every
// thread returns the same {prefix, need, done}; workgroup 0 stores it for the next launch.
__device__ __forceinline__ SelState sel_resolve(const SelState* __restrict__ st_prev, SelState* __restrict__ st_next,
                                                const uint32_t* __restrict__ hist_prev, int prev_shift, int prev_width,
                                                bool first, uint32_t n, uint32_t count, uint32_t* s_scan,
                                                SelState* s_out) {
    const int tid = threadIdx.x;
    SelState cur;
    cur.prefix = 0; cur.need = n; cur.done = 0;
    if (first) {
        const uint32_t kmax = st_prev->kmax, kmin = ~st_prev->kmin_inv;
        if (n >= count) { cur.prefix = ~0ull; cur.done = 1; }                       // every row
        else if (kmin == kmax) { cur.prefix = ((unsigned long long)kmin << 32) | (n - 1); cur.done = 1; }   // equal keys: the ring
    } else {
        cur.prefix = st_prev->prefix; cur.need = st_prev->need; cur.done = st_prev->done;
    }
    if (!cur.done) {                                        // (uniform over the grid)
        const int bins = 1 << prev_width;
        const int per = (bins + 255) / 256;
        const int b0 = tid * per, b1 = min(b0 + per, bins);
        uint32_t sum = 0;
        for (int b = b0; b < b1; ++b) sum += sel_bin(hist_prev, b);
        s_scan[tid] = sum;
        if (tid == 0) { s_out->prefix = 0; s_out->need = 0; s_out->done = 1; }     // (a histogram that holds fewer than `need`: select nothing)
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {           // inclusive scan
            const uint32_t add = tid >= off ? s_scan[tid - off] : 0u;
            __syncthreads();
            s_scan[tid] += add;
            __syncthreads();
        }
        uint32_t excl = s_scan[tid] - sum;
        if (excl < cur.need && cur.need <= excl + sum) {    // exactly one thread
            int b = b0;
            uint32_t c = sel_bin(hist_prev, b);
            while (excl + c < cur.need) { excl += c; c = sel_bin(hist_prev, ++b); }
            const uint32_t need = cur.need - excl;
            unsigned long long prefix = cur.prefix | ((unsigned long long)b << prev_shift);
            const bool done = (c == need) || prev_shift == 0;
            if (done) prefix |= (1ull << prev_shift) - 1ull;          // every row of the bin
            s_out->prefix = prefix; s_out->need = need; s_out->done = done ? 1u : 0u;
        }
        __syncthreads();
        cur.prefix = s_out->prefix; cur.need = s_out->need; cur.done = s_out->done;
    }
    if (blockIdx.x == 0 && tid == 0) { st_next->prefix = cur.prefix; st_next->need = cur.need; st_next->done = cur.done; }
    return cur;
}

__device__ __forceinline__ void sel_count(uint32_t ok, int64_t r, int64_t cursor, int64_t count, unsigned long long prefix,
                                          int prev_shift, int shift, uint32_t mask, uint32_t* s_hist) {
    const uint64_t comp = retention_comp(ok, r, cursor, count);
    if ((comp >> prev_shift) == (prefix >> prev_shift)) atomicAdd(&s_hist[(uint32_t)(comp >> shift) & mask], 1u);
}

// pass i >= 1: narrow the prefix, then histogram the digit (shift, width) of the rows that match it
__global__ __launch_bounds__(256) void select_pass_kernel(const uint32_t* __restrict__ okeys, int64_t count,
                                                          int64_t cursor, uint32_t n, int first, int prev_shift,
                                                          int prev_width, int shift, int width,
                                                          const SelState* __restrict__ st_prev,
                                                          SelState* __restrict__ st_next,
                                                          const uint32_t* __restrict__ hist_prev,
                                                          uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_hist[SEL_BINS];
    __shared__ uint32_t s_scan[256];
    __shared__ SelState s_out;
    const SelState cur = sel_resolve(st_prev, st_next, hist_prev, prev_shift, prev_width, first != 0, n, (uint32_t)count,
                                     s_scan, &s_out);
    if (cur.done) return;
    const int bins = 1 << width;
    const uint32_t mask = (uint32_t)bins - 1u;
    for (int b = threadIdx.x; b < bins; b += 256) s_hist[b] = 0;
    __syncthreads();
    const int64_t groups = count >> 2;                      // four keys per 16-byte load
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
        const uint4 k4 = reinterpret_cast<const uint4*>(okeys)[g];
        sel_count(k4.x, 4 * g, cursor, count, cur.prefix, prev_shift, shift, mask, s_hist);
        sel_count(k4.y, 4 * g + 1, cursor, count, cur.prefix, prev_shift, shift, mask, s_hist);
        sel_count(k4.z, 4 * g + 2, cursor, count, cur.prefix, prev_shift, shift, mask, s_hist);
        sel_count(k4.w, 4 * g + 3, cursor, count, cur.prefix, prev_shift, shift, mask, s_hist);
    }
    if (blockIdx.x == 0 && (int64_t)threadIdx.x < (count & 3)) {
        const int64_t r = 4 * groups + threadIdx.x;
        sel_count(okeys[r], r, cursor, count, cur.prefix, prev_shift, shift, mask, s_hist);
    }
    __syncthreads();
    sel_flush_hist(s_hist, bins, hist);
}

// The compaction's caller-owned half, `Out`:
//   bool skip(uint32_t ok, int64_t r) const       the row takes no part, whatever its composite
//   void write(uint32_t pos, int64_t r) const     the row is entry `pos` (< n) of the output, in arrival order

// a selected row goes to the workgroup's list
template <class Out>
__device__ __forceinline__ void sel_collect(uint32_t ok, int64_t r, int64_t cursor, int64_t count, unsigned long long thr,
                                            uint32_t* s_n, int32_t* s_rows, const Out& out) {
    if (out.skip(ok, r)) return;
    if (retention_comp(ok, r, cursor, count) <= thr) s_rows[atomicAdd(s_n, 1u)] = (int32_t)r;
}

// write the workgroup's list behind the rows already written (one global add), then empty it
template <class Out>
__device__ __forceinline__ void sel_write_list(uint32_t* s_n, uint32_t* s_base, const int32_t* s_rows, uint32_t n,
                                               uint32_t* __restrict__ out_count, const Out& out) {
    const uint32_t cnt = *s_n;
    if (threadIdx.x == 0 && cnt) *s_base = atomicAdd(out_count, cnt);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < cnt; i += 256) {
        const uint32_t pos = *s_base + i;
        if (pos >= n) continue;                             // (cannot happen: at most n composites are <= the threshold)
        out.write(pos, s_rows[i]);
    }
    __syncthreads();
    if (threadIdx.x == 0) *s_n = 0;
    __syncthreads();
}

// the body of a compaction kernel (256 threads): the last narrowing, then every row at or below the threshold, in
// arrival order
template <class Out>
__device__ __forceinline__ void sel_compact(const uint32_t* __restrict__ okeys, int64_t count, int64_t cursor, uint32_t n,
                                            int first, int prev_shift, int prev_width,
                                            const SelState* __restrict__ st_prev, SelState* __restrict__ st_next,
                                            const uint32_t* __restrict__ hist_prev, uint32_t* __restrict__ out_count,
                                            const Out& out) {
    __shared__ uint32_t s_scan[256];
    __shared__ SelState s_out;
    __shared__ int32_t s_rows[SEL_LIST];
    __shared__ uint32_t s_n, s_base;
    const SelState cur = sel_resolve(st_prev, st_next, hist_prev, prev_shift, prev_width, first != 0, n, (uint32_t)count,
                                     s_scan, &s_out);
    const unsigned long long thr = cur.prefix;              // (the last digit ends at bit 0: the prefix is the threshold)
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const int64_t groups = count >> 2;
    // every thread of the workgroup makes the same number of trips (barriers inside); a trip adds at most 1024 rows
    for (int64_t g0 = (int64_t)blockIdx.x * 256; g0 < groups; g0 += (int64_t)gridDim.x * 256) {
        const int64_t g = g0 + threadIdx.x;
        if (g < groups) {
            const uint4 k4 = reinterpret_cast<const uint4*>(okeys)[g];
            sel_collect(k4.x, 4 * g, cursor, count, thr, &s_n, s_rows, out);
            sel_collect(k4.y, 4 * g + 1, cursor, count, thr, &s_n, s_rows, out);
            sel_collect(k4.z, 4 * g + 2, cursor, count, thr, &s_n, s_rows, out);
            sel_collect(k4.w, 4 * g + 3, cursor, count, thr, &s_n, s_rows, out);
        }
        __syncthreads();
        const uint32_t held = s_n;                          // (read by all before anyone adds again)
        __syncthreads();
        if (held > SEL_LIST - 1024 - 4)                     // (uniform) no room for another trip and the tail
            sel_write_list(&s_n, &s_base, s_rows, n, out_count, out);
    }
    if (blockIdx.x == 0 && (int64_t)threadIdx.x < (count & 3)) {
        const int64_t r = 4 * groups + threadIdx.x;
        sel_collect(okeys[r], r, cursor, count, thr, &s_n, s_rows, out);
    }
    __syncthreads();
    sel_write_list(&s_n, &s_base, s_rows, n, out_count, out);
}

// ---- host ------------------------------------------------------------------------------------------------------
// digits of the composite: the three of the key, then the bits of the rotated row that `count` needs
inline int sel_passes(int64_t count, int* shifts, int* widths) {
    int P = 0;
    shifts[P] = 52; widths[P++] = 12;
    shifts[P] = 40; widths[P++] = 12;
    shifts[P] = 32; widths[P++] = 8;
    int s = 0;
    while (s < 31 && (1LL << s) < count) ++s;               // rotated rows are < count <= 2^s
    while (s > 0) {
        const int w = s < 12 ? s : 12;
        s -= w;
        shifts[P] = s; widths[P++] = w;
    }
    return P;
}

// workspace of a selection: [n composites (int64)] [SelState x (passes + 1)] [histograms] [ordered keys (u32 x count)]
struct SelWorkspace {
    int64_t* out_comp;
    SelState* st;
    uint32_t* hist;
    uint32_t* okeys;
    int64_t clear_bytes;                // from st on: the states and the histograms, zeroed before pass 0
};
inline int64_t sel_state_bytes() { return aura_align256((SEL_MAX_PASSES + 1) * (int64_t)sizeof(SelState)); }
inline int64_t sel_hist_bytes() { return (int64_t)SEL_MAX_PASSES * SEL_COPIES * SEL_BINS * 4; }
inline int64_t sel_workspace_bytes(int64_t count, int64_t n) {
    return aura_align256(8 * n) + sel_state_bytes() + sel_hist_bytes() + aura_align256(4 * count);
}
inline SelWorkspace sel_workspace(void* workspace, int64_t n) {
    char* w = static_cast<char*>(workspace);
    SelWorkspace ws;
    ws.out_comp = reinterpret_cast<int64_t*>(w);
    w += aura_align256(8 * n);
    ws.st = reinterpret_cast<SelState*>(w);
    ws.hist = reinterpret_cast<uint32_t*>(w + sel_state_bytes());
    ws.okeys = reinterpret_cast<uint32_t*>(w + sel_state_bytes() + sel_hist_bytes());
    ws.clear_bytes = sel_state_bytes() + sel_hist_bytes();
    return ws;
}
inline int64_t sel_blocks4(int64_t count) {
    int64_t blocks4 = (count / 4 + 255) / 256;
    if (blocks4 < 1) blocks4 = 1;
    if (blocks4 > SEL_MAX_BLOCKS) blocks4 = SEL_MAX_BLOCKS;
    return blocks4;
}

// the digit passes after the caller's pass 0 (the compaction, the caller's own kernel, narrows once more)
inline int sel_launch_passes(const SelWorkspace& ws, int64_t count, int64_t cursor, int64_t n, const int* shifts,
                             const int* widths, int P, hipStream_t s) {
    const int64_t blocks4 = sel_blocks4(count);
    for (int i = 1; i < P; ++i) {
        hipLaunchKernelGGL(select_pass_kernel, dim3((unsigned)blocks4), dim3(256), 0, s, ws.okeys, count, cursor, (uint32_t)n,
                           i == 1 ? 1 : 0, shifts[i - 1], widths[i - 1], shifts[i], widths[i], ws.st + (i - 1), ws.st + i,
                           ws.hist + (int64_t)(i - 1) * SEL_COPIES * SEL_BINS, ws.hist + (int64_t)i * SEL_COPIES * SEL_BINS);
        const int rc = aura_check_launch();
        if (rc) return rc;
    }
    return AURA_OK;
}
