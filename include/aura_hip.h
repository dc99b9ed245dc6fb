/*
 * aura_hip.h -- C ABI of libaura_hip.so: the MI355X (gfx950) implementation of Aura's
 * SNN-timestep + episodic-retrieval hot path.
 *
 * The reference (auralmn/aura-snn-rag) is 100 % Python/PyTorch and has no FFI of its own
 * (SURVEY.md section 0); the boundary it exposes for this path is the nn.Module API listed in
 * SURVEY.md section 8b.  Each entry point below names the reference method whose arithmetic it
 * replaces (file:line relative to the upstream checkout).  The Python classes in
 * aura_snn_rag_amd/ keep the reference's signatures and call these through ctypes
 * (INTEGRATION.md shows the binding a reference maintainer would add).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless it says "host";
 *   - sizes are element counts, int64_t; tensors are dense row-major;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); every call is
 *     asynchronous on that stream and never synchronises or allocates;
 *   - the return value is 0 on success, a negative AURA_E_* code otherwise; nothing throws;
 *   - all arithmetic is IEEE fp32 without FMA contraction in the neuron loops, so results are
 *     bit-identical to the reference's unfused PyTorch op sequence.
 */
#ifndef AURA_HIP_H
#define AURA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AURA_OK 0
#define AURA_E_INVAL (-1)   /* bad argument (null pointer, negative size, unsupported value) */
#define AURA_E_LAUNCH (-2)  /* HIP reported a launch error */
#define AURA_E_ALIGN (-3)   /* pointer alignment requirement violated */

#define AURA_DTYPE_F32 0
#define AURA_DTYPE_BF16 1

/* image_format: the 16-bit format of a list-sorted image of the inverted lists (and of any image that
 * aura_bank_find_repeats scans).  Any other value is AURA_E_INVAL. */
#define AURA_IMAGE_BF16 0
#define AURA_IMAGE_F16  1   /* IEEE half, conversion and rho16 as documented under "The list-sorted image in IEEE half" */

/* gif flags */
#define AURA_GIF_TIME_INVARIANT 1 /* h is [rows, H]: the same current at every timestep */
#define AURA_GIF_MEAN_OUT 2       /* out is [rows, H] = mean over T of the spikes */

/* Library identification: returns a static string "aura_hip <version> gfx950". */
const char* aura_version(void);

/* ---------------------------------------------------------------------------------------
 * Spiking-neuron membrane loops
 * ------------------------------------------------------------------------------------- */

/* Izhikevich Euler loop, time-contiguous layout I[N][T] -> spikes[N][T]; v,u [N] in/out.
 * Replaces IzhikevichNeuron._jit_step_loop, src/base/neuron.py:181-196 (2-D / 1-D inputs of
 * forward_sequence, :162-167). */
int aura_izh_run_nt(const float* I, float* spikes, float* v, float* u, float a, float b, float c,
                    float d, float dt, int64_t N, int64_t T, void* stream);

/* Same loop, channel-contiguous layout I[B][T][D] -> spikes[B][T][D]; state index b*D+d.
 * Replaces the 3-D branch of forward_sequence (permute/reshape, src/base/neuron.py:158-160,
 * 176-178) without materialising the permuted copy. */
int aura_izh_run_btd(const float* I, float* spikes, float* v, float* u, float a, float b, float c,
                     float d, float dt, int64_t B, int64_t T, int64_t D, void* stream);

/* AdEx Euler loop; params = the 11-float buffer of src/base/neuron.py:207
 * {tau_m,E_L,V_T,Delta_T,R,tau_w,a,b,V_reset,V_spike,dt} passed BY VALUE from the host.
 * Replaces AdExNeuron._jit_step_loop, src/base/neuron.py:233-248. */
int aura_adex_run_nt(const float* I, float* spikes, float* V, float* w, const float* params_host,
                     int64_t N, int64_t T, void* stream);
int aura_adex_run_btd(const float* I, float* spikes, float* V, float* w, const float* params_host,
                      int64_t B, int64_t T, int64_t D, void* stream);

/* Vectorised LIF over x[B][T][size] (T = 1 is the single step of VectorizedLIFNeuron.forward,
 * src/base/neuron.py:131-139; T > 1 is the per-t loop of EnhancedSpikingNeuron.forward,
 * src/base/snn_brain_zones.py:73-79).  beta, threshold: [size]; mem: [B][size] in/out; dtype of all five =
 * AURA_DTYPE_*.  In bf16 (a module moved to bf16: buffers, parameters, input and state) every op rounds its fp32
 * result to bf16, as the reference does. */
int aura_lif_run(const void* x, void* spikes, void* mem, const void* beta, const void* threshold,
                 int64_t B, int64_t T, int64_t size, int dtype, void* stream);

/* GIF membrane loop (decay, clamp, divide, floor-spike, soft reset, threshold adaptation).
 * h: currents after the neuron's nn.Linear, [rows][T][H] (or [rows][H] with
 * AURA_GIF_TIME_INVARIANT); out: spikes [rows][T][H] (or the T-mean [rows][H] with
 * AURA_GIF_MEAN_OUT); v, theta: [rows][H] in/out; dtype of h/out/v/theta = AURA_DTYPE_*.
 * In bf16 every op rounds to bf16, as the reference does (state dtype follows the input,
 * gif_neuron.py:46-47).  Replaces GIFNeuron.forward's loop,
 * src/core/language_zone/gif_neuron.py:54-69 (+ MultiBitSurrogate.forward :11-13) and the
 * spikes.mean(dim=1) readout of SNNFFN.forward, snn_ffn.py:81.  The mean is
 * RNE_dtype(fp32 sum / T): the spike counts summed in fp32, divided by T in fp32, rounded once
 * to the output dtype (checked against torch 2.10 on the CPU; an older torch may have differed). */
int aura_gif_run(const void* h, void* out, void* v, void* theta, float decay, int L, float alpha,
                 float threshold, int64_t rows, int64_t T, int64_t H, int dtype, int flags,
                 void* stream);

/* ---------------------------------------------------------------------------------------
 * Episodic bank (HippocampalFormation)
 * ------------------------------------------------------------------------------------- */

/* inv_norm[i] = 1 / max(||bank[row0+i]||_2, 1e-12) for i in [0, n): the per-row factor of
 * F.normalize(active_feats, dim=1), src/core/hippocampal.py:278, hoisted out of the query. */
int aura_bank_row_norms(const float* bank, float* inv_norm, int64_t row0, int64_t n, int64_t D,
                        void* stream);

/* One-shot write of n rows: bank[slots[i]] = feats[i]; loc[slots[i]] = cur_loc;
 * meta[slots[i]] = {1, now, cid, 0}; inv_norm[slots[i]] refreshed.  With centroids != NULL
 * each row is assigned to its nearest centroid among the first `eff_k` (L2), the centroid's
 * running mean and count are updated IN ROW ORDER (c <- (1-1/n)c + (1/n)x), and cid is stored;
 * otherwise cid = -1.  slots: int64 [n] device.  Replaces create_episodic_memory's tensor
 * work, src/core/hippocampal.py:211-232. */
int aura_bank_write(float* bank, float* loc, float* meta, float* inv_norm, float* centroids,
                    float* centroid_counts, int eff_k, const float* feats, const int64_t* slots,
                    const float* cur_loc, int spatial_dims, float now, int64_t n, int64_t D,
                    void* stream);

/* aura_bank_write with centroids != NULL for batches whose slots are all DISTINCT, same results bit for
 * bit: the distances leave the serial chain -- every row is scored against the table as it stands at
 * batch start in parallel, then one workgroup walks the rows in order and re-scores (with the serial
 * arithmetic) only the centroids that earlier rows of the batch moved close enough to matter
 * (hippocampal.py:218-230 is order dependent: row i sees the centroids left by rows < i).
 * workspace: aura_bank_write_online_workspace_bytes(n) bytes, 256-byte aligned. */
int64_t aura_bank_write_online_workspace_bytes(int64_t n);
int aura_bank_write_online(float* bank, float* loc, float* meta, float* inv_norm, float* centroids,
                           float* centroid_counts, int eff_k, const float* feats, const int64_t* slots,
                           const float* cur_loc, int spatial_dims, float now, int64_t n, int64_t D,
                           void* workspace, int64_t workspace_bytes, void* stream);

/* meta[i][0] *= (1 - rate) for i < count.  Replaces decay_memories, hippocampal.py:334. */
int aura_bank_decay(float* meta, float rate, int64_t count, void* stream);

/* Retention: which rows a full bank gives up first, and reinforcement of the rows a recall returned.
 * [build-side] no upstream counterpart (the reference's full bank overwrites slot 0).
 *   key(r) = meta[r][0] * expf(-(now - meta[r][1]) / 3600)          (strength x the recall's temporal factor)
 * Eviction order of rows [0, count): (key, (r - cursor) mod count) ascending, a NaN key first, -0 == +0.
 * aura_bank_retention_keys: out[r] = key(r), r < count.
 * aura_bank_select_weakest: the first n rows of the eviction order (1 <= n <= count, 0 <= cursor) by a radix
 *   select over the composite  ordered_u32(key) << 32 | rotated row : the metadata is read once (16 B per row),
 *   every further pass reads 4 B per row.  out_slots / out_keys (device, [n]) receive the n rows and their keys
 *   in the compaction's arrival order, and the first n int64 of the workspace the rows' composites with the top
 *   bit flipped (ascending as signed integers = the eviction order): sorting those n values orders the
 *   selection (ops.bank_select_weakest does).  workspace: *_workspace_bytes(count, n) bytes, 256-byte aligned.
 * aura_bank_reinforce: for every DISTINCT r in rows[0 .. n_rows) with 0 <= r < count (others are ignored):
 *   s = meta[r][0]; if (s < cap) meta[r][0] = fminf(s + amount, cap) -- once per call however often r occurs
 *   (a bitmap of count bits in the workspace, cleared by the call).  amount >= 0.
 * All three read 16-byte metadata rows: meta must be 16-byte aligned. */
int aura_bank_retention_keys(const float* meta, int64_t count, float now, float* out, void* stream);
int64_t aura_bank_select_weakest_workspace_bytes(int64_t count, int64_t n);
int aura_bank_select_weakest(const float* meta, int64_t count, float now, int64_t cursor, int64_t n,
                             int64_t* out_slots, float* out_keys, void* workspace, int64_t workspace_bytes,
                             void* stream);
int64_t aura_bank_reinforce_workspace_bytes(int64_t count);
int aura_bank_reinforce(float* meta, int64_t count, const int32_t* rows, int64_t n_rows, float amount, float cap,
                        void* workspace, int64_t workspace_bytes, void* stream);

/* Diverse recall: a greedy maximal-marginal-relevance selection of k rows among the F candidates a recall
 * returned (csrc/aura_diverse.hip).  [build-side] no upstream counterpart.
 * Per query: F candidates in rank order, cand_rows[q][j] (int32) and cand_scores[q][j] (fp32), j = 0..F-1.  A
 * candidate is valid if 0 <= row < count and its score is not NaN; the others (the -1 padding) are ignored.
 *   cos(i, j) = fp32 dot product over D of bank[row_i] * inv_norm[row_i] and bank[row_j] * inv_norm[row_j].
 *   S = the candidates picked so far, m(c) = max over j in S of cos(c, j).
 *   eligible: valid, not picked, and (S empty or m(c) < max_similarity)   (any value above 1 switches it off);
 *   value:    (1 - diversity) * score[c] while S is empty, else (1 - diversity) * score[c] - diversity * m(c);
 *   pick the eligible candidate of largest value, equal values -> the smallest j; stop after k picks or when
 *   nobody is eligible.
 * out_rows / out_scores [nq][k]: the picks in pick order, the candidates' rows and score bits; the unfilled tail is
 * row -1, score -inf.  The first pick is candidate 0; diversity = 0 with max_similarity > 1 returns candidates
 * 0..k-1 unchanged.  0 <= diversity <= 1; 1 <= k <= F <= 128; D % 4 == 0, 4 <= D <= 4096; bank 16-byte aligned.
 * One launch, no atomics; the F x F cosines live in LDS, so *_workspace_bytes is 0 for every supported shape
 * (negative for an unsupported one) and workspace may be NULL. */
int64_t aura_diverse_select_workspace_bytes(int64_t nq, int64_t F, int64_t k);
int aura_diverse_select(const float* bank, const float* inv_norm, int64_t count, int64_t D, const int32_t* cand_rows,
                        const float* cand_scores, int64_t nq, int64_t F, int64_t k, float diversity,
                        float max_similarity, float* out_scores, int32_t* out_rows, void* workspace,
                        int64_t workspace_bytes, void* stream);

/* Consolidating writes: which rows of a batch repeat a memory the bank holds, or an earlier row of the same batch
 * (csrc/aura_consolidate.hip).  [build-side] no upstream counterpart (the reference stores every row).
 * Inputs: the N held rows bank[0 .. N), a batch of n <= 1024 new rows f_0 .. f_{n-1} (feats [n][D]) and a threshold
 * tau in (0, 1].
 *   cos(x, y) = the dot product of the two rows, each scaled by 1 / max(||.||, 1e-12), evaluated in fp32; bank rows
 *     use the stored inv_norm.  Any fp32 evaluation within (D + 8) 2^-24 of the exact value is acceptable, so two
 *     evaluations differ by at most tol = 2 (D + 8) 2^-24: decisions closer than tol to tau, or between two targets
 *     closer than tol to each other, may fall either way.
 *   stored_target[i] = the held row r of largest cos(f_i, r) if that cosine is >= tau, else -1; bit-identical bank
 *     rows tie to the lowest r.  The search covers EVERY held row and is exact, whatever image is passed.
 *   batch_leader: walk i = 0 .. n-1 in order.  A row with a stored target is a repeat and never a leader.  Among the
 *     others, row i repeats the KEPT earlier row j < i of largest cos(f_i, f_j) >= tau (ties -> the lowest j):
 *     batch_leader[i] = j; otherwise row i is kept and batch_leader[i] = -1.
 *   cos_out[i] = the cosine to whatever row i repeats, -inf for a kept row.
 *   A row with a NaN or Inf component and a row of norm 0 are kept and are nobody's target (their cosines are NaN
 *     or 0).  The norm is the fp32 one: a batch row whose SQUARED norm overflows fp32 (||f|| > 1.8e19) or underflows
 *     to 0 (||f|| < 1e-23) counts as such a row.
 * The scan.  image != NULL: a CURRENT 16-bit image of the normalised held rows ([n_image][D], D % 8 == 0, D <= 768,
 *   16-byte aligned) in `image_format` -- the row-ordered bf16 shadow (image_rows == NULL, n_image = N: image row i is
 *   bank row i) or the list-sorted image of the inverted lists (image_rows = sorted_rows, n_image = n_sorted; -1
 *   entries are padding or holes) -- with rho [rows of the bank], the residual norms of THIS image: rho as
 *   aura_bank_shadow_update leaves it for AURA_IMAGE_BF16, the image's rho16 for AURA_IMAGE_F16.  One pass over the
 *   image on the 16-bit matrix pipe against the batch's normalised rows in the same format; a pair survives when
 *   cos_16 + err >= tau with the prefilter's bound err = rho_row + rho_q + rho_row rho_q + 2 D 2^-24 + 1e-5
 *   (aura_knn_search_ex); survivors go to per-row lists of 256 entries and a second launch re-scores them in fp32 from
 *   the fp32 bank.  A list that overflows sets *overflow_out (device int32, reset by every call) to non-zero: the
 *   results are then incomplete and the caller repeats the call with image == NULL.
 *   image == NULL: a dense fp32 scan of the fp32 bank (any D <= 4096), the per-row maximum by a packed
 *   (ordered cosine bits, ~row) 64-bit atomicMax; it cannot overflow.  image_format must still be a valid value.
 * The n x n cosines of the batch are computed in fp32 on the matrix pipe (lower triangle); only rows that have a
 *   pair >= tau among rows without a stored target enter the ordered walk.
 * stored_target, batch_leader: int32 [n]; cos_out: fp32 [n]; workspace: *_workspace_bytes(n) bytes (negative for an
 * unsupported n), 256-byte aligned.  Nothing is written to the bank.
 *
 * Consolidation within tags: batch_tags != NULL selects the scoped search -- two more inputs and nothing else of the
 * rule changed.  batch_tags == NULL: the scope-blind search above; meta is then ignored.
 *   meta [rows of the bank][4]: the bank's metadata; column 3 holds the tag as a float, read as
 *     aura_knn_search_scoped reads it (a value outside (-1, 2^24) is no tag and matches nothing).
 *   batch_tags int32 [n], on the device: one tag per batch row.
 * Eligibility.  A held row r < N is eligible for batch row i iff (int)meta[r][3] == batch_tags[i]; an in-batch pair
 *   (i, j) is eligible iff batch_tags[i] == batch_tags[j].  Tag 0, "untagged", is a scope like any other.  A batch tag
 *   outside [0, 2^24) matches nothing -- no held row and no other batch row, not even one with the same value -- so
 *   that row is kept and is nobody's leader.
 * Results.  stored_target[i] = the ELIGIBLE held row of largest cosine >= tau, bit-identical rows tie to the lowest
 *   eligible r; the ordered walk considers only KEPT earlier rows of the same tag.  The cosine, the degenerate rows,
 *   cos_out and tol = 2 (D + 8) 2^-24 are unchanged.  Equivalently: the rule above applied to cosine matrices in which
 *   every ineligible pair is -inf.
 * All three scans take the predicate where a pair is decided, never afterwards: the image scan before a survivor is
 *   appended to a list (rows of other tags cannot fill the 256 entries; with a list-sorted image the tag is that of bank
 *   row image_rows[ir], read from meta, so the image needs no upkeep when a tag changes), the dense scan before the
 *   packed atomicMax, the Gram before a row is marked pending, the walk before a kept row offers its cosine.  The
 *   overflow flag, the workspace and every other argument are unchanged.  AURA_E_INVAL also for batch_tags != NULL
 *   with meta == NULL and N > 0; AURA_E_ALIGN for a meta or batch_tags that is not 4-byte aligned.
 * aura_bank_touch: meta[r][1] = now for every 0 <= r < count among rows[0 .. n) (int32; others are ignored;
 *   duplicates store the same value). */
int64_t aura_bank_find_repeats_workspace_bytes(int64_t n);
int aura_bank_find_repeats(const float* bank, const float* inv_norm, int64_t N, int64_t D, const uint16_t* image,
                           const int32_t* image_rows, int64_t n_image, const float* rho, const float* feats, int64_t n,
                           float tau, int32_t* stored_target, int32_t* batch_leader, float* cos_out,
                           int32_t* overflow_out, void* workspace, int64_t workspace_bytes, const float* meta,
                           const int32_t* batch_tags, int image_format, void* stream);
int aura_bank_touch(float* meta, int64_t count, const int32_t* rows, int64_t n, float now, void* stream);

/* Blending merges: a repeated memory moves toward the rows that repeat it (csrc/aura_blend.hip).  [build-side] the
 * reference's centroid index keeps an online running mean of what it absorbs (hippocampal.py:226-228); its bank stores
 * every row.
 *
 * THE RULE.  Inputs: the stored_target / batch_leader of ONE aura_bank_find_repeats call (scoped or not) for a batch
 * f_0 .. f_{n-1} (n <= 1024) against the N held rows, and a rate beta in (0, 1], fp32.
 *   Group key of batch row i.  stored_target[i] = r >= 0: held row r.  Else batch_leader[i] = j >= 0: batch row j.
 *     Else row i is kept and is a member of nothing.
 *   Members are never keys (a row with a stored target or a leader is not stored); they are read unblended.
 *   Held key r.  g = bank[r]; for its members in ASCENDING i:  g = g + beta * (f_i - g), per component in fp32 with
 *     three roundings -- the difference, the product, the sum; never fused (-ffp-contract=off and the pragma of
 *     aura_common.inl).  Then bank[r] = g.  The order matters: the update does not commute for beta != 1/2.
 *   Batch key j.  The same chain from g = f_j; the result replaces row j of the batch as it will be stored.
 *   Decisions.  Every decision of the call is the one find_repeats made against the bank as it stood BEFORE the blend:
 *     a blended memory that drifts within tau of another held memory merges with it only at the next consolidate().
 *   Metadata.  Strength, timestamp, tag, centroid id, ids and centroid_counts are not touched; reinforcing, touching
 *     and the maxima of consolidate() stay what they are.  The stored centroid id and the centroid means stay until the
 *     next centroid rebuild, as after a compaction.
 *
 * aura_bank_blend applies the rule in one launch and keeps the derived state of every BANK row it moves current:
 *   bank[r]; inv_norm[r] with aura_bank_row_norms' arithmetic, bit for bit; when shadow_bf16 is given and
 *   r < shadow_upto, shadow_bf16[r] and rho[r] with aura_bank_shadow_update's arithmetic; when the list-sorted image is
 *   given and pos_of_row[r] = p with 0 <= p < n_sorted and sorted_rows[p] == r, the row in `image_format` into image[p]
 *   (for AURA_IMAGE_BF16 the same bf16 bits; rho[r] receives the bf16 residual either way, and with AURA_IMAGE_F16
 *   rho16[r], when rho16 is not NULL, the half image's), in place -- the centroid id has not changed, so the lists
 *   gain no hole and use no slack.  A cached table of aura_ivf2_row_constants is stale afterwards (rho changed).
 * The batch.  feats_row0 == -1: feats [n][D]; blended batch keys go to out_feats [n][D], which the caller has filled
 *   with a copy of feats (only blended rows are written; feats itself never is); the write that stores them derives
 *   their norms and shadows as for any row.  feats_row0 >= 0: the batch IS bank rows [feats_row0, feats_row0 + n)
 *   (feats / out_feats are ignored); held targets lie below it (N <= feats_row0) and a blended batch key is written
 *   in place with the derived state above.
 * Grouping is done on the device from the two arrays (device int32 [n]); nothing is read back.  Every id is checked
 *   before it becomes an address: a stored target outside [0, N), and a leader outside [0, i) or one that is not
 *   itself a kept row, are ignored (the row is a member of nothing).  Sets no flag, needs no workspace, cannot overflow.
 * 1 <= D <= 4096; n == 0 launches nothing.  16-byte accesses when D % 4 == 0 and bank is 16-byte aligned (the
 *   condition of aura_bank_row_norms, so that the norm associates alike), 4-byte ones otherwise.
 * AURA_E_INVAL: n outside [0, 1024], D outside [1, 4096], rows < N or rows >= 2^31, beta outside (0, 1] or NaN,
 *   feats_row0 < -1 or a slab outside [N, rows], a null array that is needed, rho given without shadow_bf16 or the
 *   image (or the reverse), the image's three arrays not all given, an image or shadow with D % 8 != 0, shadow_upto
 *   outside [0, rows], an image_format that is not one, rho16 with AURA_IMAGE_BF16.  AURA_E_ALIGN: a shadow or image
 *   that is not 16-byte aligned or comes with an unaligned bank; an aligned bank with D % 4 == 0 whose feats /
 *   out_feats are not 16-byte aligned. */
int aura_bank_blend(float* bank, float* inv_norm, int64_t N, int64_t rows, int64_t D, const float* feats,
                    int64_t feats_row0, int64_t n, const int32_t* stored_target, const int32_t* batch_leader,
                    float beta, float* out_feats, uint16_t* shadow_bf16, float* rho, int64_t shadow_upto,
                    uint16_t* image, float* rho16, const int32_t* sorted_rows, const int32_t* pos_of_row,
                    int64_t n_sorted, int image_format, void* stream);

/* In-place compaction of the bank (csrc/aura_compact.hip): the primitive under forgetting, pruning and the
 * consolidation of held rows.  [build-side] no upstream counterpart (the reference's pruning ends in `pass`).
 * For every i < n, row src[i] of every array moves to row dst0 + i.  The arrays: bank [rows][D], loc [rows][S],
 * meta [rows][4], inv_norm [rows] and, when given, the row-ordered bf16 shadow [rows][D] and rho [rows] (both or
 * neither; a shadow needs D % 8 == 0).  src (device int32 [n]) ascends strictly and dst0 + i <= src[i] < rows.
 * The result is as if every source row were read before any destination is written.  Rows outside dst0 .. dst0 + n - 1
 * are not written (the caller clears the freed tail).  A row with dst0 + i == src[i] causes no traffic.
 * Rows are taken in rounds of aura_bank_compact_round_rows() = 4096 in ascending order.  A round whose whole
 * destination range lies below its first source goes straight to its place (one read and one write per byte); any
 * other round is gathered into one half of the workspace and stored from it by the next launch, which also takes the
 * next round: rounds + 1 launches per call, all on the caller's stream, no allocation, no host synchronisation (the
 * device decides from src which kind a round is).  n == 0 launches nothing.
 * 16-byte accesses when D % 4 == 0 and bank is 16-byte aligned, 4-byte ones otherwise.  An entry of src that breaks
 * dst0 + i <= src[i] < rows is skipped before it becomes an address; an order that does not ascend gives an
 * unspecified arrangement of in-range rows.
 * workspace: *_workspace_bytes(D, S, has_shadow) bytes -- two halves of 4096 rows of every array, independent of rows
 * and n; negative for an unsupported shape (1 <= D <= 4096, 0 <= S <= 4096) -- 256-byte aligned.
 * AURA_E_INVAL: a null array, shadow without rho or the reverse, a negative size, dst0 + n > rows, rows >= 2^31,
 * a workspace that is too small; AURA_E_ALIGN: workspace not 256-byte, shadow not 16-byte, another array not 4-byte
 * aligned. */
int64_t aura_bank_compact_round_rows(void);
int64_t aura_bank_compact_workspace_bytes(int64_t D, int64_t S, int has_shadow);
int aura_bank_compact(float* bank, float* loc, float* meta, float* inv_norm, uint16_t* shadow_bf16, float* rho,
                      int64_t rows, int64_t D, int64_t S, const int32_t* src, int64_t n, int64_t dst0, void* workspace,
                      int64_t workspace_bytes, void* stream);

/* Scoped recall: tags on memories and the exact top-k over a per-query subset of the held rows
 * (csrc/aura_scoped.hip).  [build-side] no upstream counterpart (the reference accepts event_id and drops it;
 * column 3 of its memory_metadata is "reserved").
 * A tag is an integer in [0, 2^24) held as a float in meta[r][3]; 0 = untagged, what every write leaves there.
 * aura_bank_set_tags: meta[slots[i]][3] = (float)tags[i] for i < n, plain vector stores; an entry with a slot outside
 *   [0, count) or a tag outside [0, 2^24) is skipped before it becomes an address.  slots (device int64 [n]) must be
 *   distinct (the caller keeps the last write to a slot); tags device int32 [n].  One launch; n == 0 launches nothing.
 * aura_knn_search_scoped.  Row r < count is in query i's scope iff ALL of
 *     tag_i < 0  or  (int)meta[r][3] == tag_i                       (tag_i = -1: any tag; 0: the untagged rows)
 *     conditions & 1 == 0  or  meta[r][1] >= newer_than             (fp32 comparisons on the stored fp32 timestamps,
 *     conditions & 2 == 0  or  meta[r][1] <= older_than              which are 128 s apart at today's epoch values)
 *     conditions & 4 == 0  or  meta[r][0] >= min_strength
 *   hold; rows at or beyond count never match, whatever their column 3 holds.  Per query the result is the top k rows
 *   of its scope by the combined score of aura_knn_search ((0.5 cos + 0.3 spatial + 0.2 exp(-(now - ts) / 3600)) *
 *   strength, the same fp32 arithmetic; q_loc == NULL: spatial = 0), descending, equal scores -> the lower row; a scope
 *   of fewer than k rows leaves the tail at score -inf, row -1.  Always exact over the scope; the centroid index plays
 *   no part.  The score bits of a (query, row) pair do not depend on which other queries or rows share the call: the
 *   dot product is accumulated in one fixed order along D (v_mfma_f32_32x32x2_f32, exact fp32).
 *   The plan (device int32, built by the host, which knows the queries' tags): with S = n_scopes distinct scopes and
 *   T = n_tiles query tiles,
 *     plan[0 .. S)            the scopes' tags, strictly ascending, "any tag" = -1 first when a query uses it;
 *     plan[S .. S + T)        tile_scope: the scope (index) of every query tile;
 *     plan[S + T .. S + 2T)   tile_q0, plan[S + 2T .. S + 3T) tile_nq: the tile's queries are
 *                             q_order[tile_q0 .. tile_q0 + tile_nq), 1 <= tile_nq <= 64, all of ONE scope;
 *     plan[S + 3T .. + nq)    q_order: the query indices grouped by scope (a permutation of 0 .. nq - 1).
 *   S <= 256 per call (a caller with more distinct tags chunks its queries), 1 <= k <= 128, 1 <= splits <= 64,
 *   1 <= count < 2^30, 1 <= D <= 4096 (16-byte loads when D % 4 == 0 and bank and queries are 16-byte aligned, 4-byte
 *   loads otherwise); meta 16-byte aligned; spatial_dims <= 4 with q_loc.
 *   The launches: query norms; a count pass over meta[0 .. count) (16 B per row) per block of 256 rows; an exclusive
 *   prefix over blocks and scopes; a scatter pass that leaves every scope's row ids in ascending order (a stable
 *   compaction: no atomic decides a position, the order does not depend on the launch geometry); the scan, grid
 *   (T, splits): a tile's queries against their scope's gathered rows, 128 at a time, split s taking row tiles s,
 *   s + splits, ..., each query's sorted top-k kept in registers; for splits > 1 a merge of the splits' lists.  The work
 *   of the scan follows sum_i |scope(i)| / 64, not the bank.  Nothing is read back between the launches, nothing is
 *   allocated: workspace is *_workspace_bytes(count, nq, k, n_scopes, splits) bytes (negative: unsupported), 256-byte
 *   aligned.
 *   *flag_out (device int32, reset by every call): bit 0 = a scope list held a row id outside [0, count) (skipped
 *   before it became an address), bit 1 = the plan named a scope, tile or query that does not exist (that tile is
 *   skipped).  Either means the results are not to be trusted; neither can fault. */
int aura_bank_set_tags(float* meta, int64_t count, const int64_t* slots, const int32_t* tags, int64_t n, void* stream);
int64_t aura_knn_scoped_workspace_bytes(int64_t count, int64_t nq, int64_t k, int64_t n_scopes, int64_t splits);
int aura_knn_search_scoped(const float* bank, const float* inv_norm, const float* meta, const float* loc,
                           int spatial_dims, const float* queries, const float* q_loc, float now, int64_t count,
                           int64_t D, int64_t nq, int k, const int32_t* plan, int64_t n_scopes, int64_t n_tiles,
                           int64_t splits, int conditions, float newer_than, float older_than, float min_strength,
                           float* out_scores, int32_t* out_rows, void* workspace, int64_t workspace_bytes,
                           int32_t* flag_out, void* stream);

/* Per-tag quotas: a tag at its limit gives up its OWN weakest memories (csrc/aura_quota.hip, and the masked form of
 * the selection above in csrc/aura_bank.hip).  [build-side] no upstream counterpart.
 *
 * THE RULE.  A bank under overflow='weakest' may carry a quota q(t) >= 1 for some tags t (a "limited" tag; tags without
 * a quota are unlimited).  Terms:
 *   key(r)            = meta[r][0] * expf(-(now - meta[r][1]) / 3600), the arithmetic of aura_bank_retention_keys;
 *   eviction order of tag t: its rows of [0, count) by (key, (r - c_t) mod count) ascending, a NaN key first, -0 == +0;
 *   c_t               the tag's TIE ORIGIN, kept on the host per limited tag, 0 at first.  (Stored timestamps are fp32,
 *                     128 s apart: rows written within two minutes tie.  Ranked from the bank's one cursor, the row a
 *                     tag has just overwritten would be first in ring order again: the tag would churn one slot and
 *                     keep its oldest rows.  With its own origin behind its last victim a tag of tied keys is a FIFO.)
 * A batch is cut into runs; a run holds at most q(t) rows of each limited tag t (the longest such prefix, on top of the
 * cuts the write path makes anyway) and is ranked once, from the rows held before it.  For one run of n rows, in_t of
 * them of limited tag t, held_t rows of [0, count) carrying t, M the bank's capacity:
 *   1. tag victims    x_t = min(in_t, max(0, held_t + in_t - q(t))): the first x_t rows of t's eviction order;
 *                     then c_t <- (the last of them) + 1.
 *   2. appends        rem = n - sum_t x_t,  n_app = min(rem, M - count).
 *   3. global victims g = rem - n_app: the first g rows of the bank's usual eviction order (the global cursor) among
 *                     the rows that are NOT tag victims of this run; then cursor += g.
 *   4. slots          the run's first n_app rows append; the others overwrite, in this order: the tag victims, scopes in
 *                     ascending tag order, each scope in its own eviction order; then the global victims in theirs.
 * Consequences: a quota is a cap, not a reservation (a full bank may take a global victim from a tag under its quota);
 * a tag over its quota (after a bulk or positioned write, a retag, a lowered quota, a loaded checkpoint: none of them
 * enforce quotas) neither grows nor shrinks on writes until the host takes the first held_t - q(t) rows of its
 * eviction order out; rows a consolidating write merges are not stored and do not count.
 *
 * aura_bank_tag_counts: out[s] (device int32 [n_scopes]) = the number of rows r < count with (int)meta[r][3] ==
 *   scope_tags[s] (a column 3 outside (-1, 2^24) carries no tag).  scope_tags: device int32, distinct, strictly
 *   ascending (the caller's duty: a list that is not finds fewer rows, never a wrong address), 1 <= n_scopes <=
 *   AURA_QUOTA_MAX_SCOPES.  One pass over the metadata, counts in LDS, one integer add per workgroup and non-empty
 *   scope.  count == 0 zeroes out and launches nothing.  Needs no workspace.
 * aura_bank_select_weakest_scoped: for up to AURA_QUOTA_MAX_SCOPES scopes at once, with origin[s], incoming[s] and
 *   quota[s] (device int32 [n_scopes]; a quota beyond int32 is as good as 2^31 - 1): computes held_s and
 *   x_s = min(incoming, max(0, held + incoming - quota), held) on the device and selects EXACTLY the first x_s rows of
 *   scope s's eviction order (step 1 above) by one radix select with n_scopes thresholds over
 *   ordered_u32(key) << 32 | (r - origin[s]) mod count, 8-bit digits: the metadata is read once (16 B per row), every
 *   further pass reads 8 B per row.  out_held / out_x (device int64 [n_scopes]); scope s owns the entries
 *   [off_s, off_s + incoming[s]) of out_slots / out_comp (device int64 [out_capacity], off_s = sum of incoming[j],
 *   j < s; out_capacity >= the sum of incoming, entries beyond it are never written): its x_s rows in arrival order,
 *   each with its composite, top bit flipped (ascending as signed integers = the scope's eviction order), then -1 /
 *   INT64_MAX.  Sorting a scope's entries by composite orders its selection.  Sets bit r of bitmap (device uint32
 *   [(count + 31) / 32], caller-held, NOT cleared by the call: several calls over disjoint scope subsets share one
 *   bitmap when a run carries more than 64 limited tags; the scopes' victim sets are disjoint, so the grouping does not
 *   matter) for every selected row r.  Integer adds and ors only: nothing depends on arrival order but the order within
 *   a scope's output range.  workspace: *_workspace_bytes(count, n_scopes), 256-byte aligned.
 * aura_bank_select_weakest_masked: aura_bank_select_weakest among the rows whose bitmap bit is clear (step 3 above).
 *   n must not exceed the number of such rows (fewer: the remaining entries of out_slots / out_keys are not written).
 *   The same kernels as the unmasked selection, instantiated with the mask; same outputs, same workspace size.
 * AURA_E_INVAL / AURA_E_ALIGN as for aura_bank_select_weakest, and for n_scopes outside [1, 64], a null array, a
 * negative out_capacity; nothing is launched then. */
#define AURA_QUOTA_MAX_SCOPES 64
int aura_bank_tag_counts(const float* meta, int64_t count, const int32_t* scope_tags, int64_t n_scopes, int32_t* out,
                         void* stream);
int64_t aura_bank_select_weakest_scoped_workspace_bytes(int64_t count, int64_t n_scopes);
int aura_bank_select_weakest_scoped(const float* meta, int64_t count, float now, const int32_t* scope_tags,
                                    const int32_t* origin, const int32_t* incoming, const int32_t* quota,
                                    int64_t n_scopes, int64_t out_capacity, int64_t* out_held, int64_t* out_x,
                                    int64_t* out_slots, int64_t* out_comp, uint32_t* bitmap, void* workspace,
                                    int64_t workspace_bytes, void* stream);
int64_t aura_bank_select_weakest_masked_workspace_bytes(int64_t count, int64_t n);
int aura_bank_select_weakest_masked(const float* meta, int64_t count, float now, int64_t cursor, int64_t n,
                                    const uint32_t* bitmap, int64_t* out_slots, float* out_keys, void* workspace,
                                    int64_t workspace_bytes, void* stream);

/* Replay: a seeded draw of held memories by priority, without replacement (csrc/aura_replay.hip).  [build-side] the
 * reference samples a Python list of CPU tensors (hippocampal_trainer.py:43-66, torch.randperm); its bank cannot be
 * sampled.
 *
 * THE RULE.  For a call (count, now, priority, alpha, scope, seed, draw, n), rows r < count, all fp32, unfused:
 *   1. random word    x_r = word 0 of Philox4x32-10 with counter (r & 0xffffffff, r >> 32, draw & 0xffffffff, draw >> 32)
 *                     and key (seed & 0xffffffff, seed >> 32); multipliers 0xD2511F53, 0xCD9E8D57, key increments
 *                     0x9E3779B9, 0xBB67AE85 (Random123; counter 0, key 0 gives 6627e8d5).
 *   2. uniform        u_r = ((x_r >> 9) + 0.5) * 2^-23: a 24-bit odd numerator over 2^24, exact in fp32, inside
 *                     [2^-24, 1 - 2^-24]: never 0 or 1.
 *   3. log-priority   lw_r = logf(meta[r][0]) + a with a = -(now - meta[r][1]) / 3600   (AURA_REPLAY_KEY: the log of the
 *                            retention key; a is the argument aura_bank_retention_keys hands to expf.  In the log domain
 *                            on purpose: expf underflows for rows older than about four days, which would never be drawn)
 *                          = logf(meta[r][0])                                          (AURA_REPLAY_STRENGTH)
 *                          = 0                                                         (AURA_REPLAY_UNIFORM)
 *   4. eligible       r is in scope and lw_r is finite (KEY, STRENGTH: 0 < strength < inf; KEY: a timestamp that is not
 *                     NaN).  Does not depend on alpha.  In scope iff ALL of
 *                       n_tags == 0 (any tag)  or  the row's tag (column 3, as aura_knn_search_scoped reads it: a value
 *                                                   outside (-1, 2^24) is no tag) is one of tags[0 .. n_tags), 0 = untagged
 *                       conditions & 1 == 0  or  meta[r][1] >= newer_than
 *                       conditions & 2 == 0  or  meta[r][1] <= older_than
 *                       conditions & 4 == 0  or  meta[r][0] >= min_strength
 *   5. draw key       d_r = alpha * lw_r - logf(-logf(u_r)), 0 <= alpha <= 16; a zero is written as +0.
 *   6. sample         the first n' = min(n, #eligible) eligible rows by (d descending, row ascending), in that order;
 *                     then rows -1 and keys -inf up to n.
 * This is the exponential-race form of successive sampling (Gumbel top-n).  With p = exp(alpha lw):
 *   - the first row is r with probability p_r / sum p; each later row is drawn the same way from what is left;
 *   - the first m rows of a sample of n are the sample of m;
 *   - the sample of a scope is the full-bank order filtered to that scope;
 *   - the key of a (draw, row) pair does not depend on what else is in the call, on n, or on the launch geometry.
 *
 * tags: HOST int32 [n_tags], 0 <= n_tags <= AURA_REPLAY_MAX_TAGS, each in [0, 2^24), strictly ascending (they travel in
 *   the kernel arguments; the call reads them before it returns).  meta: 16-byte aligned.
 * aura_bank_replay_keys: out_d[r] = d_r for r < count, -inf for an ineligible row; out_u (may be NULL) [count] receives
 *   the 23-bit integers x_r >> 9.  One pass, reads 16 B per row.  count == 0 launches nothing.
 * aura_bank_replay: out_rows (int32 [n]) / out_d (fp32 [n]) receive the sample's n' rows and keys in the compaction's
 *   arrival order, the other n - n' entries the padding (written on the device: the host never learns n'), and the first
 *   n int64 of the workspace the composites  ~ordered_u32(d) << 32 | row  with the top bit flipped, INT64_MAX for the
 *   padding (ascending as signed integers = the sample's order): sorting those n values orders the sample
 *   (ops.bank_replay does).  out_eligible (int64 [1]) = #eligible.  The key pass is pass 0 of the radix selection of
 *   aura_bank_select_weakest (16 B per row once, then 4 B per row per pass; the same digit passes and compaction).
 *   1 <= n <= count; workspace: *_workspace_bytes(count, n) bytes, 256-byte aligned.  count == 0: any n >= 1, writes
 *   the padding with fills and launches nothing (workspace size 0).
 * AURA_E_INVAL, nothing launched: n < 1 or n > count; alpha outside [0, 16] or NaN; an unknown priority; n_tags outside
 *   [0, 64], a tag outside [0, 2^24) or tags not strictly ascending; conditions with unknown bits; a null array; a
 *   workspace that is too small.  AURA_E_ALIGN: meta not 16-byte, workspace not 256-byte, an output not aligned to its
 *   element. */
#define AURA_REPLAY_KEY 0
#define AURA_REPLAY_STRENGTH 1
#define AURA_REPLAY_UNIFORM 2
#define AURA_REPLAY_MAX_TAGS 64
int aura_bank_replay_keys(const float* meta, int64_t count, float now, int priority, float alpha, const int32_t* tags,
                          int64_t n_tags, int conditions, float newer_than, float older_than, float min_strength,
                          uint64_t seed, uint64_t draw, float* out_d, uint32_t* out_u, void* stream);
int64_t aura_bank_replay_workspace_bytes(int64_t count, int64_t n);
int aura_bank_replay(const float* meta, int64_t count, float now, int priority, float alpha, const int32_t* tags,
                     int64_t n_tags, int conditions, float newer_than, float older_than, float min_strength,
                     uint64_t seed, uint64_t draw, int64_t n, int32_t* out_rows, float* out_d, int64_t* out_eligible,
                     void* workspace, int64_t workspace_bytes, void* stream);

/* Workspace size (bytes) aura_knn_search needs for (N, nq, k). */
int64_t aura_knn_workspace_bytes(int64_t N, int64_t nq, int k);

/* Exact batched recall: for each of nq queries the top-k rows of bank[0..N) by the reference's
 * combined score (0.5*cos + 0.3*spatial + 0.2*exp(-(now-ts)/3600)) * strength, descending,
 * ties -> lower row index.  q_loc == NULL means "no location" (spatial = 0).
 * Outputs: out_scores [nq][k] fp32, out_idx [nq][k] int32 (row index + idx_base).
 * k <= min(N, 1024).  workspace: aura_knn_workspace_bytes(N, nq, k) bytes of HBM.
 * Replaces retrieve_similar_memories steps 1-5, src/core/hippocampal.py:272-307, for a batch
 * of queries (the reference is called once per batch row,
 * memory_augmented_layer.py:113-121). */
int aura_knn_search(const float* bank, const float* inv_norm, const float* meta, const float* loc,
                    int spatial_dims, const float* queries, const float* q_loc, float now,
                    int64_t N, int64_t D, int64_t nq, int k, int32_t idx_base, float* out_scores,
                    int32_t* out_idx, void* workspace, int64_t workspace_bytes, void* stream);

/* As aura_knn_search with extras: centroids != NULL restricts each query's candidates to the rows
 * whose centroid id (meta[.][2]) is among the `nprobe` nearest (L2, unnormalised query) of the
 * 256 centroid rows -- the candidate selection of retrieve_similar_memories,
 * src/core/hippocampal.py:259-270 (a query left without candidates returns idx -1 everywhere and
 * the caller falls back to the full scan, :269-270); flags (AURA_KNN_FORCE_DENSE scores every row densely instead
 * of using the sampled-threshold filter; same results, used by tests) and overflow_out (device
 * int32, reset by every call and set non-zero if a candidate list overflowed -- bit 0: filter
 * list of the fp32 scan, bit 2 / bit 3: candidate / survivor list of the two-stage path, bit 4: a
 * candidate row id outside [0, N) reached the re-scoring stage (an internal invariant broke; the row
 * is dropped instead of dereferenced) -- the caller must then re-run with AURA_KNN_FORCE_DENSE; may
 * be NULL). */
/* overflow_out bit 6: some query of a two-stage call ended with NO candidate row at all (its probed
 * centroids own no rows): its outputs are -inf / -1 and the caller applies the reference's full-scan
 * fallback (hippocampal.py:269-270).  Not an overflow: the other queries' results are complete. */
#define AURA_KNN_FLAG_NO_CANDIDATES 64
/* overflow_out bit 7 (aura_knn_search_ivf2): the caller's lists_flag was set -- aura_ivf2_append dropped
 * a row because its list had no free entry left: the lists must be re-packed and the call repeated. */
#define AURA_KNN_FLAG_LISTS_STALE 128
#define AURA_KNN_FORCE_DENSE 1
/* AURA_KNN_FP32_SCAN: score every row on the fp32 matrix pipe.  Without it, large banks
 * (>= 8192 rows, D <= 768, D % 4 == 0, no location term / centroid mask, k <= 256) are first
 * filtered by a bf16 scan whose error is bounded rigorously (round-to-nearest bf16 of both
 * operands: |cos_bf16 - cos_fp32| <= rho_row + rho_query + rho_row rho_query + 2 D 2^-24 + 1e-5
 * with rho <= 2^-8 the relative L2 rounding residuals), and only rows that can still reach the top
 * k are re-scored in fp32 with the same arithmetic: results are bit-identical either way. */
#define AURA_KNN_FP32_SCAN 2
int aura_knn_search_ex(const float* bank, const float* inv_norm, const float* meta,
                       const float* loc, int spatial_dims, const float* queries,
                       const float* q_loc, float now, int64_t N, int64_t D, int64_t nq, int k,
                       int32_t idx_base, float* out_scores, int32_t* out_idx, void* workspace,
                       int64_t workspace_bytes, int flags, int32_t* overflow_out,
                       const float* centroids, int nprobe, void* stream);

/* Inverted-list (IVF) form of the centroid-candidate recall: identical results to
 * aura_knn_search_ex(..., centroids, nprobe) without a location term, but each probed list is
 * streamed once per pass of up to 2048 queries and only against the queries that probe it.
 * list_rows: row ids of bank[0..N) grouped by centroid id (int32 [N], rows with centroid id < 0
 * first); list_off [257]: start of each list in list_rows (list_off[256] = N); list_len [256].
 * The host module derives the three arrays from meta[.][2] after writes / rebuilds.  nprobe <= 8.
 * cap: candidate slots per query, a multiple of 2048 with (cap/2048)*k <= 16384; the sum of the
 * nprobe longest lists never overflows it.  A query whose lists hold more rows sets *overflow_out
 * (the caller falls back to the masked full scan).
 * workspace: aura_knn_ivf_workspace_bytes(nq, k, cap) bytes.
 * Replaces retrieve_similar_memories steps 0-5, src/core/hippocampal.py:259-307. */
int64_t aura_knn_ivf_workspace_bytes(int64_t nq, int k, int cap);
int aura_knn_search_ivf(const float* bank, const float* inv_norm, const float* meta,
                        const float* queries, float now, int64_t N, int64_t D, int64_t nq, int k,
                        const float* centroids, int nprobe, const int32_t* list_rows,
                        const int32_t* list_off, const int32_t* list_len, int cap,
                        int32_t idx_base, float* out_scores, int32_t* out_idx, void* workspace,
                        int64_t workspace_bytes, int32_t* overflow_out, void* stream);

/* Measurement hooks (bench.py): between aura_profile_begin(max) and aura_profile_end, every
 * launch of the main scan kernel inside aura_knn_search[_ex] is bracketed by HIP events recorded
 * on the launch stream.  aura_profile_end synchronises those events, writes up to max_out
 * per-launch durations in milliseconds to the HOST array and returns how many it wrote
 * (negative AURA_E_* on error). */
int aura_profile_begin(int max_launches);
/* Tuning hook (tools/ab_headline.py): replaces the AURA_CS_DBG ablation flags of the scan kernels for the
 * following calls (flags < 0: only read) and returns the previous value.  Non-zero flags switch kernel phases
 * off or on for timing experiments; results are only valid with 0, the default. */
int aura_debug_cs_flags(int flags);
/* Tuning hook: the shader clock in MHz as a kernel sees it (s_memtime ticks per 100-MHz s_memrealtime tick over
 * spin_us microseconds, 1..100000), written to out_dev[0] (device float). */
int aura_debug_clock_mhz(float* out_dev, int spin_us, void* stream);
int aura_profile_end(float* ms_out_host, int max_out);
/* Bank rows and queries scored by the most recent profiled main-scan launch (HOST pointers):
 * the units behind bench.py's algorithmic FLOP count, 2 * rows * nq * D per launch. */
int aura_profile_last_scan(int64_t* rows_out, int64_t* nq_out);
/* 0 = the profiled launch was the fp32 matrix scan, 1 = the bf16 prefilter scan over the fp32 bank,
 * 2 = the prefilter scan over the bf16 shadow, 3 = the inverted-list prefilter scan (sorted shadow). */
int aura_profile_last_scan_kind(void);

/* Merge S per-shard top-k lists into the global top-k (the step after the RCCL all-gather,
 * SURVEY.md section 8e).  in_scores/in_idx: [S][nq][k]; out: [nq][k]; ties -> lower index. */
int aura_topk_merge(const float* in_scores, const int32_t* in_idx, int S, int64_t nq, int k,
                    float* out_scores, int32_t* out_idx, void* stream);

/* k-means-lite pieces of rebuild_centroids, src/core/hippocampal.py:358-376.
 * assign: assign_out[i] = argmin_c ||bank[i] - centroids[c]|| over the first k centroids
 *   (computed as argmin |c|^2 - 2 x.c on the fp32 matrix cores; ties -> lower c);
 *   cnorm2_ws: k floats of scratch.
 * segment_means: the masked means of :358-363 as a segmented reduction.  The caller groups the rows
 *   by cluster (a stable sort of assign): order [N] int32 row ids, seg_off [k+1] int32 with
 *   order[seg_off[c] .. seg_off[c+1]) = rows of cluster c.  centroids[c] = mean of those rows, summed
 *   in a fixed order (reproducible); empty clusters keep their centroid (:362-363).  With sums_only
 *   the per-cluster SUMS are written instead (zeros for empty clusters): a rank's partial result
 *   of a row-sharded bank, all-reduced with the counts.  Reads the bank once.
 *   N == 0: every cluster is empty -- with sums_only the first k rows become zeros, else nothing is written.
 *   The order is a tested contract (tests/index_rule.py segment_sum32): per chunk of 64 rows of the segment four
 *   accumulators take rows r, r+1, r+2, r+3 while four remain, the rest go to the first, s = (a0 + a1) + (a2 + a3);
 *   the chunks are added in order from zero; the mean is that sum divided by float(len), rounded once.
 *   D % 4 == 0; workspace: aura_kmeans_means_workspace_bytes(N, D, k) bytes, 16-byte aligned.
 * commit: meta[i][2] = assign[i] for i < N and counts[c] = seg_off[c+1] - seg_off[c] (counts may be
 *   NULL) -- the recount / metadata write of :370-376. */
int aura_kmeans_assign(const float* bank, const float* centroids, float* cnorm2_ws,
                       int32_t* assign_out, int64_t N, int64_t D, int k, void* stream);
int64_t aura_kmeans_means_workspace_bytes(int64_t N, int64_t D, int k);
int aura_kmeans_segment_means(const float* bank, const int32_t* order, const int32_t* seg_off, float* centroids,
                              void* workspace, int64_t workspace_bytes, int64_t N, int64_t D, int k,
                              int sums_only, void* stream);
int aura_kmeans_commit(const int32_t* assign, const int32_t* seg_off, float* meta, float* counts, int64_t N,
                       int k, void* stream);

/* Gather rows: out[i] = bank[idx[i]] (idx outside [0, rows) -> zeros; rows = rows of the bank); used
 * to return [B,k,D] memory features (memory_augmented_layer.py:124-128). */
int aura_bank_gather(const float* bank, int64_t rows, const int32_t* idx, float* out, int64_t n, int64_t D,
                     void* stream);

/* Optional bf16 shadow of the bank for the two-stage recall's prefilter (halves the bytes the
 * prefilter streams; results unchanged: the survivors are still re-scored from the fp32 bank).
 * [build-side] no upstream counterpart; the product keeps it beside memory_features
 * (src/core/hippocampal.py:88) exactly as it keeps 1/||row||.
 * A shadow row is the NORMALISED row rounded to bf16: bank_bf16[r] = bf16(bank[r] * inv_norm[r]);
 * rho[r] (fp32, [rows of the bank]) is an upper bound of its L2 rounding residual against the unit
 * row -- the row's part of the prefilter's error bound, measured instead of assumed (<= 2^-8).
 * aura_bank_shadow_update: rows r in slots[0..n) (device int64) or, with slots == NULL,
 * [row0, row0 + n); inv_norm must be current for them.  D % 8 == 0, both bases 16-byte aligned. */
int aura_bank_shadow_update(const float* bank, const float* inv_norm, uint16_t* bank_bf16, float* rho,
                            const int64_t* slots, int64_t row0, int64_t n, int64_t D, void* stream);

/* aura_knn_search_ex without location term, with the shadow (bank_bf16 == NULL: same as
 * aura_knn_search_ex).  bank_bf16 / rho must be current (aura_bank_shadow_update) for every r < N.
 * centroids / nprobe as in aura_knn_search_ex: with the shadow the centroid-candidate restriction
 * (hippocampal.py:259-270) is applied inside the two-stage scan (probe masks in LDS) instead of the
 * fp32 scan. */
int aura_knn_search_shadow(const float* bank, const uint16_t* bank_bf16, const float* rho, const float* inv_norm,
                           const float* meta, const float* queries, float now, int64_t N, int64_t D,
                           int64_t nq, int k, int32_t idx_base, float* out_scores, int32_t* out_idx,
                           void* workspace, int64_t workspace_bytes, int flags, int32_t* overflow_out,
                           const float* centroids, int nprobe, void* stream);

/* Centroid-index recall (hippocampal.py:259-270) as inverted lists on the two-stage machinery: the
 * caller keeps a LIST-SORTED 16-bit image of the bank, bf16 or IEEE half -- `image_format` says which, one
 * argument of every function below -- sorted row i holds the shadow row of bank row sorted_rows[i] (-1: no
 * row, scanned as padding), the rows of one centroid contiguous.
 * pad_off [257]: first sorted row of each list, multiples of 16 (pad_off[256] <= n_sorted);
 * list_len [256]: entries in use, list_len[c] <= pad_off[c+1] - pad_off[c] -- the difference is
 * slack that aura_ivf2_append fills after writes, so the lists are re-packed only when the centroids
 * are rebuilt; every entry beyond list_len[c] must be -1.
 * aura_bank_shadow_sorted converts all n_sorted rows (and refreshes rho[row]; pos_of_row, if not NULL,
 * receives the reverse map bank row -> sorted row for aura_ivf2_append).
 * aura_ivf2_append: after a write of n DISTINCT bank rows `slots` (device int64) whose centroid ids
 * are in meta[.][2]: the row's previous entry becomes a hole (-1), the row is appended to its list
 * (image row converted, rho refreshed, pos_of_row updated).  A row whose list has no free entry left is
 * dropped from the lists and *flag |= 1: pass that flag to aura_knn_search_ivf2 as lists_flag (it is
 * reported as AURA_KNN_FLAG_LISTS_STALE) or re-pack after at most `slack` appended rows.
 * aura_centroid_probe: ids_out[q][p] (p < nprobe, [nq][8] int32) = the p-th nearest of the 256 centroid
 * rows to query q (L2 on the unnormalised query, ties to the lower row: hippocampal.py:261-262), exactly
 * what aura_knn_search_ivf2 computes for itself; workspace: aura_centroid_probe_workspace_bytes(nq)
 * bytes, 256-byte aligned.
 * row_constants (optional, [n_sorted][4] fp32, 16-byte aligned): the sorted rows' score constants
 * {0.5 strength, temporal term + error, temporal term - error, bank row id bits} -- the per-row half of
 * hippocampal.py:290-303's combined score as the prefilter bounds it.  They depend on the bank's metadata,
 * rho, the list layout and `now` only, so a caller may build them once with aura_ivf2_row_constants(now)
 * and pass them to every search that uses the SAME `now` (fp32: the reference's fp32 timestamps give it a
 * 128-second grain) until metadata or layout change; aura_ivf2_append keeps a table current for the
 * entries it touches (pass the table and its `now`; NULL: no table).  NULL in the search: computed per
 * call into the workspace.
 *
 * The list-sorted image in IEEE half (AURA_IMAGE_F16).  Normalised rows and queries lie in [-1, 1], so half (11
 * significand bits) covers them at the size of bf16 (8 bits) and the prefilter's band U - L = 2 (rho_row + E_fix + eq)
 * becomes 5-6 times narrower at D = 768: fewer candidates leave the filter scan and fewer survivors are gathered in
 * fp32 by the refine.  Results are unchanged (the rows and score bits of the fp32 scan).
 *   Conversion: fl(bank[r] * inv_norm[r]) rounded to nearest, ties to even; an element with |x| < 2^-14 is stored as
 *     +0, so the image holds no subnormal and the bound does not depend on how the matrix pipe treats them; the
 *     residual is taken against what is stored.  Queries are converted alike.
 *   rho16 [rows of the bank]: the residual norm of the half image, aura_bank_shadow_update's formula on that residual.
 *     The writers (aura_bank_shadow_sorted, aura_ivf2_append, aura_bank_blend) keep writing the bf16 residual into
 *     `rho` bit for bit as they do for a bf16 image (the row-ordered shadow shares that array) and write rho16 when it
 *     is not NULL.  The readers (aura_ivf2_row_constants, aura_knn_search_ivf2, the aura_bank_find_repeats scan) take
 *     rho16 in rho's place.  aura_ivf2_append with a table of row constants needs rho16.  With AURA_IMAGE_BF16 rho16
 *     must be NULL (AURA_E_INVAL otherwise).
 *   Negative strengths use their own worst-case query bound, (1.001 (2^-11 1.00001 + sqrt(D) 2^-14) + (D/2 + 3) 2^-24)
 *     (1 + 2^-7): 2^-11 relative on the elements that stay normal, at most 2^-14 each on those stored as 0.
 * Every other argument, limit and return code is the same for both formats. */
/* `rho`: the residual norms of THIS image -- rho for AURA_IMAGE_BF16, rho16 for AURA_IMAGE_F16. */
int aura_ivf2_row_constants(const float* meta, const float* rho, const int32_t* sorted_rows, int64_t n_sorted,
                            int64_t D, float now, float* row_constants, int image_format, void* stream);
int64_t aura_knn_ivf2_workspace_bytes(int64_t n_sorted, int64_t nq, int k);
int64_t aura_centroid_probe_workspace_bytes(int64_t nq);
int aura_centroid_probe(const float* centroids, const float* queries, int64_t D, int64_t nq, int nprobe,
                        int32_t* ids_out, void* workspace, int64_t workspace_bytes, void* stream);
int aura_bank_shadow_sorted(const float* bank, const float* inv_norm, const int32_t* sorted_rows, uint16_t* image,
                            float* rho, float* rho16, int32_t* pos_of_row, int64_t n_sorted, int64_t D,
                            int image_format, void* stream);
int aura_ivf2_append(const float* bank, const float* inv_norm, const float* meta, const int64_t* slots,
                     int64_t n, int64_t D, uint16_t* image, int32_t* sorted_rows, const int32_t* pad_off,
                     int32_t* list_len, int32_t* pos_of_row, float* rho, float* rho16, int32_t* flag,
                     float* row_constants, float row_constants_now, int image_format, void* stream);

/* One layout of the inverted lists, as described above; what ops.Ivf2Lists validates once.  Pointers and 64-bit
 * fields first, the two 32-bit ints last: no interior padding. */
typedef struct aura_ivf2_lists {
    const float* bank;                /* [N][D] fp32, 16-byte aligned */
    const float* inv_norm;            /* [N] */
    const float* meta;                /* [N][4], 16-byte aligned; the centroid ids are in meta[.][2] */
    const float* centroids;           /* [256][D] */
    const uint16_t* image;            /* [n_sorted][D] in image_format, 16-byte aligned */
    const float* rho;                 /* [N]: residual norms of THIS image (rho16 for AURA_IMAGE_F16) */
    const int32_t* sorted_rows;       /* [n_sorted]: the sorted rows' bank rows, all < N; -1: padding or a hole */
    const int32_t* pad_off;           /* [257] */
    const int32_t* list_len;          /* [256] */
    const int32_t* lists_flag;        /* optional: aura_ivf2_append's flag, reported as AURA_KNN_FLAG_LISTS_STALE */
    const float* row_constants;       /* optional, 16-byte aligned, for exactly the `now` of the call */
    int64_t n_sorted;                 /* sorted rows in use: a multiple of 16, > 0 */
    int64_t N;                        /* rows of the bank */
    int64_t D;                        /* D % 8 == 0, D <= 768 */
    int32_t nprobe;                   /* 1..8 */
    int32_t image_format;             /* AURA_IMAGE_BF16 or AURA_IMAGE_F16 */
} aura_ivf2_lists;

/* The recall: each probed list is streamed once per 256 of the queries that probe it, in passes of up to 8192
 * queries; results (rows, score bits) equal aura_knn_search_ivf's.  k <= 256; overflow_out as in aura_knn_search_ex
 * (non-zero: re-run aura_knn_search_ivf or the masked scan); workspace: aura_knn_ivf2_workspace_bytes(n_sorted, nq,
 * k) bytes, 256-byte aligned; queries [nq][D] fp32, 16-byte aligned.  nq == 0 launches nothing.
 *
 * probe_ids (optional, [nq][8] int32): aura_centroid_probe's ids of the same queries and centroid table, taken
 * instead of recomputing them: a bank sharded over ranks that share one centroid table probes every query once, on
 * the rank that owns it, not once per rank.  NULL: the call computes the probes.
 *
 * The completion word.  host_word != NULL (stage 0 only, overflow_out required): the call also tells the HOST when
 * it is done and what its flag is, without a device-to-host copy: host_word is 64 bytes of host-mapped memory from
 * aura_host_word_alloc; a one-thread launch behind the call's last kernel stores the flag into host_word[0] and then
 * host_seq into host_word[1].  The caller polls host_word[1] == host_seq (choose a new host_seq per call) and reads
 * the flag from host_word[0]; results are then final on the stream as after any launch.  One call in flight per
 * host_word.  (The flag read costs the reference-style caller a stream synchronisation per recall otherwise:
 * hippocampal.py's retrieval is synchronous too, every .item() in :311-317 waits for the GPU.)
 *
 * The recall in stages (stage != 0; stage 0 is the whole recall, k2 and bounds are then unused), for a bank that is
 * row-sharded over ranks: the prefilter's threshold of a query is a lower bound of its k-th best score,
 * and bounds found on different shards can be combined before any shard filters -- every shard then keeps about 1/S
 * of the candidates and survivors it would keep against its own bound.
 *   stage 1: everything up to the sampled bounds; bounds[q][0] = the k-th, bounds[q][1] = the k2-th
 *            (1 <= k2 <= k; 0: same as k) largest sampled lower bound of query q on THIS bank: at least k
 *            (k2) distinct rows of this bank score at least that.
 *   stage 2: same arguments, same workspace (untouched in between), bounds[q] = ONE float per query: any valid
 *            lower bound of the query's global k-th best score, e.g. max(max over shards of bounds[.][0],
 *            min over shards of bounds[.][1]) with S k2 >= k; thresholds are raised to it, then filter + refine.
 *   stage 4 + stage 3 (instead of stage 2, a second combination over the shards): stage 4 is stage 2 up to the
 *            filter scan; bounds (room for [nq][2]) carries the combined bound in its first nq floats on entry and
 *            the FILTERED CANDIDATES' bounds on return -- bounds[q][0] = the k-th, [q][1] = the k2-th largest lower
 *            bound among this bank's candidates of query q (-inf where there are fewer).  Combined like stage 1's
 *            they are close to the global k-th best score itself.  Stage 3: bounds[q] = that combination (one
 *            float per query); the refine re-scores only candidates whose upper bound reaches it, so a shard
 *            returns the rows of its top k that can be in the global top k and -1 for the rest.
 * probe_ids may be NULL (probes computed in stage 1).  nq <= 8192 per staged call; bounds is required.
 *
 * Refusals, in this order: lists == NULL (AURA_E_INVAL); a row_constants that is not 16-byte aligned (AURA_E_ALIGN);
 * an image_format that is not one, a stage outside 0..4, host_word with overflow_out == NULL or stage != 0
 * (AURA_E_INVAL); then the sizes (AURA_E_INVAL), nq == 0 (AURA_OK), a NULL required pointer (AURA_E_INVAL), the
 * alignments (AURA_E_ALIGN), n_sorted % 16 and the workspace size (AURA_E_INVAL), the staged conditions
 * (AURA_E_INVAL). */
int aura_knn_search_ivf2(const aura_ivf2_lists* lists, const float* queries, float now, int64_t nq, int k,
                         const int32_t* probe_ids, int32_t idx_base, float* out_scores, int32_t* out_idx,
                         void* workspace, int64_t workspace_bytes, int32_t* overflow_out, int stage, int k2,
                         float* bounds, uint32_t* host_word, uint32_t host_seq, void* stream);
int aura_host_word_alloc(void** host_word_out);
int aura_host_word_free(void* host_word);
/* The completion signal of aura_knn_search_ivf2 on its own: a one-thread launch on `stream` stores *flag_dev
 * (0 if NULL) into host_word[0], then host_seq into host_word[1].  For call chains that end in a call without one
 * (the staged recall): poll instead of a stream synchronisation. */
int aura_signal_flag(const int32_t* flag_dev, uint32_t* host_word, uint32_t host_seq, void* stream);

/* ---------------------------------------------------------------------------------------
 * Surrogate-gradient training path and the prosody-modulated GIF ([rows][T][H] layout)
 *
 * One entry point per operation; `dtype` = AURA_DTYPE_F32 or AURA_DTYPE_BF16 is the element type of every tensor
 * argument declared void* (bf16: bit patterns), any other value is AURA_E_INVAL.  g_gains and raw_slope are fp32
 * in both forms.  The bf16 form is the module moved to bf16 with .bfloat16() / .to(torch.bfloat16): buffers,
 * parameters, input, state AND gains are bf16 and every forward op rounds its fp32 result to bf16 (Python scalars
 * enter as fp32), which the forward kernels reproduce bit for bit (spikes and state are aura_gif_run's; save_a /
 * save_theta / pre are the bf16 values the reference's graph holds).  The backward kernels evaluate the fp32 chains
 * on the saved values with the forward's roundings re-applied to the recomputed intermediates, carry state
 * gradients in fp32 over the T steps and round once on the way out (the reference's bf16 autograd rounds every
 * intermediate gradient instead).  The GIF loops take L <= 256 in bf16 (spike counts up to 256 are exact there).
 * (A bf16 input to an fp32 module, or fp32 gains with a bf16 input, promote to fp32 in the reference: the host
 * runs those in fp32.)
 * ------------------------------------------------------------------------------------- */

/* GIF loop for training: as aura_gif_run (no flags) and additionally saves, per step, the
 * pre-clamp membrane potential (save_a) and the threshold the step started from (save_theta),
 * both [rows][T][H].  Forward of GIFNeuron.forward when autograd is recording,
 * src/core/language_zone/gif_neuron.py:54-69. */
int aura_gif_train_forward(const void* h, void* spikes, void* v, void* theta, void* save_a, void* save_theta,
                           float decay, int L, float alpha, float threshold, int64_t rows, int64_t T, int64_t H,
                           int dtype, void* stream);

/* Backward of that loop (BPTT over T): g_spikes [rows][T][H] in; g_h [rows][T][H] out; g_v,
 * g_theta [rows][H]: in = gradients of the final state, out = gradients of the initial state.
 * Spike gradient = MultiBitSurrogate.backward (triangular window, gif_neuron.py:16-22); the
 * clamp with tensor bounds routes the gradient of clamped values to theta, as autograd does. */
int aura_gif_backward(const void* save_a, const void* save_theta, const void* g_spikes, void* g_h, void* g_v,
                      void* g_theta, float decay, int L, float alpha, float threshold, int64_t rows, int64_t T,
                      int64_t H, int dtype, void* stream);

/* LIF step for training: spikes, mem_out as aura_lif_run (T = 1) plus pre = beta*mem + x - thr
 * (the surrogate's input), all [B][size]; mem_in is not modified. */
int aura_lif_train_forward(const void* x, const void* mem_in, const void* beta, const void* threshold, void* spikes,
                           void* mem_out, void* pre, int64_t B, int64_t size, int dtype, void* stream);

/* Backward of the LIF step with LearnableSurrogateGradient.backward (src/base/neuron.py:80-108):
 * g_x, g_mem_prev [B][size] and raw_slope [B][size], fp32 in both forms (sum it over the batch to get d/d slope). */
int aura_lif_backward(const void* pre, const void* g_spikes, const void* g_mem, const void* beta,
                      const void* threshold, const void* slope, void* g_x, void* g_mem_prev, float* raw_slope,
                      int64_t B, int64_t size, int dtype, void* stream);

/* ProsodyModulatedGIF.forward loop, src/core/language_zone/prosody_gif.py:69-106: gains [rows][T]
 * (NULL = no modulation) scale the input, the effective threshold (x clamp(1 - strength*(g-1),
 * 0.5, 1.5)) and the adaptation rate; no 1e-6 in the division (unlike GIFNeuron). */
int aura_gif_prosody_run(const void* h, const void* gains, void* spikes, void* v, void* theta, float decay, int L,
                         float alpha, float threshold, float strength, int64_t rows, int64_t T, int64_t H, int dtype,
                         void* stream);

/* Training forward / backward of that loop: as aura_gif_train_forward / aura_gif_backward with the
 * gains; additionally g_gains [rows][T], fp32 in both forms, receives dL/d gains (ZEROED by the caller; channels
 * are summed with float atomics; the caller rounds it): through the input gain, the threshold scale (where its
 * clamp is inactive) and the adaptation rate.  h = the currents of the forward pass.  Backward of
 * prosody_gif.py:69-106 with MultiBitSurrogate (gif_neuron.py:16-22). */
int aura_gif_prosody_train_forward(const void* h, const void* gains, void* spikes, void* v, void* theta, void* save_a,
                                   void* save_theta, float decay, int L, float alpha, float threshold, float strength,
                                   int64_t rows, int64_t T, int64_t H, int dtype, void* stream);
int aura_gif_prosody_backward(const void* save_a, const void* save_theta, const void* h, const void* gains,
                              const void* g_spikes, void* g_h, float* g_gains, void* g_v, void* g_theta, float decay,
                              int L, float alpha, float threshold, float strength, int64_t rows, int64_t T, int64_t H,
                              int dtype, void* stream);

/* ---------------------------------------------------------------------------------------
 * Brain-zone projection
 * ------------------------------------------------------------------------------------- */

/* out[b][o] = -sum_k |x[b][k] - weight_patterns[o][k]| (+ bias[o] if bias != NULL).
 * Replaces AdditionLinear.forward, src/maths/addition_linear.py:42-67, the in/out projection of
 * NeuromorphicBrainZone.forward (src/base/snn_brain_zones.py:139,161). */
int aura_addition_linear(const float* x, const float* weight_patterns, const float* bias,
                         float* out, int64_t B, int64_t in_features, int64_t out_features,
                         void* stream);

/* Backward of that projection, as autograd derives it from src/maths/addition_linear.py:50-64 (abs -> sign, with
 * sign(0) = 0):  g_x[b][k] = -sum_o g_out[b][o] sgn(x[b][k] - w[o][k]),  g_w[o][k] = +sum_b g_out[b][o] sgn(x[b][k] -
 * w[o][k]).  g_x [B][in] and g_w [out][in] are optional (NULL = not wanted); the bias gradient is g_out summed over
 * the batch (the caller's reduction). */
int aura_addition_linear_backward(const float* x, const float* weight_patterns, const float* g_out,
                                  float* g_x, float* g_w, int64_t B, int64_t in_features,
                                  int64_t out_features, void* stream);

/* ---------------------------------------------------------------------------------------
 * STDP
 * ------------------------------------------------------------------------------------- */

/* Timestep spike-timing-dependent plasticity of one dense synapse W [O][I] (csrc/aura_stdp.hip).  [build-side] the
 * reference's Synapsis keeps a rate rule on time-mean activity (src/core/language_zone/synapsis.py: "Full STDP would
 * require timestep-by-timestep update"); this is that update.
 * For batch row b and step t = 0 .. T-1, with presynaptic value pre[b,t,i], postsynaptic spike post[b,t,o] and the
 * carried traces x[b,i], y[b,o] (fp32; zero when no incoming trace is given):
 *     x[b,t,i]  = fl( fl(lambda_pre  * x[b,t-1,i]) + pre[b,t,i] )   fp32, two roundings, never fused
 *     y-[b,t,o] = fl(lambda_post * y[b,t-1,o])                      y at step t before the step's own spike: post
 *                                                                   activity strictly before t, decayed to t
 *     y[b,t,o]  = fl( y-[b,t,o] + post[b,t,o] )
 *     dW[o,i]   = (1/B) sum_b sum_t ( a_plus * post[b,t,o] * x[b,t,i]  -  a_minus * y-[b,t,o] * pre[b,t,i] )
 *     W'[o,i]   = clamp( W[o,i] + lr * dW[o,i], w_min, w_max )
 * A post spike is potentiated by the pre trace INCLUDING the same step (the synapse transmitted at t); a pre spike is
 * depressed by the post trace BEFORE the step's own spike: simultaneous spikes are potentiation only, and one pre spike
 * d steps after (before) one post spike gives -a_minus lambda_post^d / B (+a_plus lambda_pre^d / B).  pre / post may be 0/1
 * spikes, the GIF loops' levels 0 .. L or any real value.  The traces are exact fp32 recursions: every evaluation gives
 * the bits of the two-rounding form above.  dW is accumulated in fp32 by v_mfma_f32_32x32x2_f32 (bitwise a k-ordered
 * fmaf chain) over the operands a_plus * post and -a_minus * y- (one rounding each), x and pre; the batch rows are
 * split over workgroups, the splits are added in ascending order and the sum is divided by B.  The order is a function
 * of (B, T, I, O) alone: no float atomics, no dependence on the device; the same call gives the same bits every time.
 * Against the fp64 sum of the same fp32 traces, with S[o,i] = (1/B) sum_b sum_t (|a_plus post x| + |a_minus y- pre|):
 *     |dW - dW_64| <= (2 B T + 8) 2^-24 S      (and dW == 0 exactly where S == 0).
 *
 * pre  [B][T][I], or [B][I] with AURA_STDP_PRE_TIME_INVARIANT (the same value at every step);  post [B][T][O];
 *   both of `dtype` (AURA_DTYPE_F32 or AURA_DTYPE_BF16; bf16 is widened exactly).  Inputs are never written.
 * x_in [B][I], y_in [B][O]: the incoming traces, NULL = zero.  x_out, y_out: the traces after step T-1, NULL = not
 *   wanted; each element is written once.  An incoming trace must not be the array that is written.
 * W [O][I] fp32 is updated in place; with dw_out [O][I] also given, the dW that was applied is written there.  With
 *   AURA_STDP_NO_APPLY only dw_out is written (W is ignored and may be NULL; lr and the bounds are unused), with the
 *   bits an applying call writes.
 * workspace: *_workspace_bytes(B, T, I, O) = align256(splits * O * I * 4) bytes, 256-byte aligned (negative for an
 *   unsupported shape); splits = clamp(1024 / (ceil(I/128) ceil(O/128)), 1, min(B, 64)).  Two launches on `stream`.
 * AURA_E_INVAL: B < 1, T < 1, I or O not a positive multiple of 4 (either dtype), O * I > 2^40, another dtype or
 *   flag, a null pre / post / workspace, a null W when applying or a null dw_out when not, w_min > w_max or a NaN
 *   bound when applying, x_in == x_out or y_in == y_out, a workspace that is too small.  AURA_E_ALIGN: workspace not
 *   256-byte, pre / post / W / dw_out not 16-byte, a trace not 4-byte aligned. */
#define AURA_STDP_PRE_TIME_INVARIANT 1
#define AURA_STDP_NO_APPLY 2
int64_t aura_stdp_workspace_bytes(int64_t B, int64_t T, int64_t I, int64_t O);
int aura_stdp_update(const void* pre, const void* post, const float* x_in, const float* y_in, float* x_out,
                     float* y_out, float* W, float* dw_out, float lambda_pre, float lambda_post, float a_plus,
                     float a_minus, float lr, float w_min, float w_max, int64_t B, int64_t T, int64_t I, int64_t O,
                     int dtype, int flags, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Place code
 * ------------------------------------------------------------------------------------- */

/* The sparse place-cell code of PlaceCellSemanticEncoder.forward (src/core/language_zone/place_cell_encoder.py:
 * topk, sigmoid, scatter, Linear(P -> D), residual) in one launch, from the logits (csrc/aura_place.hip).  All fp32:
 * z [N][P] the logits, e [N][D] the token embeddings, W2t [P][D] the TRANSPOSE of place_to_semantic.weight, b2 [D].
 *   winners  the k winners of row n are its exact top k under this order: the larger value first; -0.0 and +0.0 are
 *            equal; a NaN (either sign) ranks above +inf, as in torch.topk, and all NaNs are equal; equal values go
 *            to the LOWER cell index (torch.topk leaves this open).  They are emitted in ASCENDING cell index:
 *            idx [N][k] int32, act [N][k].
 *   act      = 1 / (1 + expf(-z)), accurate expf (1 ulp), one add, one correctly rounded division.
 *   out      acc = 0;  for the winners j in ascending cell index: acc = fmaf(act_j, W2t[j][d], acc);
 *            r = acc + b2[d];  out[n][d] = e[n][d] + fl(0.1f * r)       (the product rounded before the add).
 *   dense    [N][P] or NULL (not wanted): +0.0 everywhere except act at the winners; every element is written.
 * A row's result depends on nothing else in the call: its bits are the same computed alone or in any batch, whatever
 * the launch geometry.  One wave owns a row: the selection is a 32-step bisection on the monotone key of the float
 * bits with the row in registers (counts by ballot), the compaction a running ballot prefix in cell order.  No atomics.
 * Against the fp64 evaluation of the same fp32 inputs with the same winners, mag = sum_j |act_j W2t[j][d]| + |b2[d]|:
 *     |act - act_64| <= 2^-22,     |out - out_64| <= 0.1 (k + 2) 2^-24 mag + 2^-23 |out_64|.
 * AURA_E_INVAL: N < 0 or N > 2^31 - 1, k < 1, k > min(P, 256), P > 8192, D < 1, D > 2^31 - 1, a null pointer other
 *   than dense.  AURA_E_ALIGN: a pointer not 4-byte aligned.  N == 0 launches nothing.  Rows move as float4 when
 *   D % 4 == 0 and e, W2t, b2 and out are 16-byte aligned, else one float at a time (the same bits). */
int aura_place_code(const float* z, const float* e, const float* W2t, const float* b2, int64_t N, int64_t P, int64_t D,
                    int64_t k, int32_t* idx, float* act, float* out, float* dense_or_null, void* stream);

/* The mirror launch: the gradient of the logits from that of out and (optionally) of the dense code.  Per row n and
 * winner j = idx[n][r], r = 0 .. k-1:
 *     dot     = <g_out[n], W2t[j]> in fp32: lane l of the row's wave owns the elements d with (d / 4) % 64 == l
 *               (d % 64 == l when the rows do not move as float4) and chains them in ascending d with fmaf from 0
 *               within each tile of 1024 (256) elements; a tile's 64 lane sums are added by the xor butterfly 32, 16,
 *               8, 4, 2, 1; the tiles' sums are added in ascending order.  The order is a function of D (and of the
 *               float4 condition below) alone.
 *     g_act   = fl(0.1f * dot)  (+ g_dense[n][j] when g_dense is given)
 *     g_z[n][j] = fl(fl(g_act * act) * fl(1 - act)),  act = act[n][r]
 * and g_z[n][c] = +0.0 at every other cell: the whole row is written.  idx must hold, per row, k ascending cells in
 * [0, P) (what aura_place_code wrote); a cell outside that range is clamped into it for the reads.  The remaining
 * gradients (g_e = g_out, g_b2 = 0.1 sum_n g_out, g_W2 = 0.1 g_out^T dense) are the caller's library calls.
 * Against fp64 on the same inputs, at a winner:
 *     |g_z - g_z64| <= (D + 3) 2^-24 * 0.1 * sum_d |g_out[n][d] W2t[j][d]| * 0.25 + 2^-23 |g_z64|   (g_dense NULL).
 * Errors as aura_place_code; float4 when D % 4 == 0 and g_out and W2t are 16-byte aligned.  One launch on `stream`. */
int aura_place_code_backward(const float* g_out, const float* g_dense_or_null, const int32_t* idx, const float* act,
                             const float* W2t, int64_t N, int64_t P, int64_t D, int64_t k, float* g_z, void* stream);

/* ---------------------------------------------------------------------------------------
 * Theta-gamma
 * ------------------------------------------------------------------------------------- */

/* The positional phase code of ThetaGammaPositionalEncoding (src/core/language_zone/theta_gamma_encoding.py) and the
 * two lines that consume it in both models' forward, h = semantic + pos and LayerNorm(h) (hippocampal_transformer.py:
 * 95-101, snn_rag_transformer.py:132-135), csrc/aura_theta.hip.  All fp32, every operation rounded on its own (no fused
 * multiply-add), fl() = round to nearest even.  For a token at position p (an fp32 number) and column d:
 *     denom = float(max(max_seq_len - 1, 1))            the module's max_seq_len, not the length of the call
 *     phi   = fl(fl(p / denom) * TWO_PI)                a correctly rounded division; TWO_PI = fp32(2 pi)
 *     a     = fl(phi + theta_off[d])
 *     g     = fl(fl(phi * ratio) + gamma_off[d])        ratio = fp32(double(gamma_freq) / double(theta_freq))
 *     A     = fl(fl(cos a + 1) * 0.5)
 *     q     = fl(sin a + fl(0.5 * fl(A * sin g)))
 *     pe    = fl(q * amp[d])
 * with the accurate sinf / cosf (full range reduction: a phase is about 32 rad at the end of max_seq_len with 8 Hz /
 * 40 Hz and thousands of radians in generation beyond it).  The derivatives of pe, from the same a, g, A:
 *     d_amp = q,   d_theta = fl(amp * fl(cos a - fl(fl(0.25 sin a) * sin g))),   d_gamma = fl(amp * fl(fl(0.5 A) * cos g)).
 * Against fp64 on the same fp32 a and g, with E = 2^-21 (4 ulp of a sine):
 *     |pe - pe_64| <= |amp| (1.75 E + 9 * 2^-24) + 2^-24 |pe_64|, and the same form for d_theta, d_gamma (d_amp: amp = 1).
 *
 * positions [R] fp32 or NULL: position r is float(start + r).  pe and the three derivative tables are [R][D]; pe may be
 * NULL when the derivatives are given, the derivatives are given all three or not at all.  One launch; sines and
 * cosines are evaluated here only, R * D times.
 * AURA_E_INVAL: R < 0 or R > 2^31 - 1, D < 1 or D > 2048, max_seq_len < 1, a null parameter vector, nothing to write.
 * AURA_E_ALIGN: a pointer not 4-byte aligned.  R == 0 launches nothing. */
int aura_theta_gamma_table(const float* positions_or_null, int64_t start, int64_t R, int64_t D, const float* theta_off,
                           const float* gamma_off, const float* amp, int64_t max_seq_len, float ratio,
                           float* pe_or_null, float* d_theta_or_null, float* d_gamma_or_null, float* d_amp_or_null,
                           void* stream);

/* y = LayerNorm(x + pe) in one launch; h is never written.  x [N][D] the tokens of B sequences of S (N = B S), table
 * [R][D]: token n reads row n % S when R == S (shared positions) and row n when R == N.  Per token:
 *     h    = fl(x + pe)
 *     mu   = sum_d h / D,   var = sum_d fl(fl(h - mu)^2) / D        (two passes over registers, biased)
 *     rstd = 1 / sqrt(var + eps)                                     (sqrt and division correctly rounded)
 *     n    = fl(fl(h - mu) * rstd),   y = fl(fl(n * w[d]) + b[d])
 * A row sum: one wave owns the token; lane l owns the units u with u % 64 == l, a unit being four consecutive columns
 * when D % 4 == 0 and one column otherwise; the lane adds its elements in ascending d from 0, the 64 lane sums are added
 * by the xor butterfly 32, 16, 8, 4, 2, 1, the total is divided by float(D).  The order is a function of D alone: a
 * token's bits are the same alone, in any batch and at any grid.  No atomics.  Writes y [N][D], mean [N] = mu, rstd [N].
 * With T_D = ceil(units / 64) * (4 or 1) + 7 and A = mean_d |h|, against fp64 on the fp32 h:
 *     |n - n_64| <= (T_D + 8) 2^-24 (A rstd + 2 |n|),    |y - y_64| <= |w| (that) + 2^-23 |y_64|.
 * AURA_E_INVAL: N < 0 or N > 2^31 - 1, D < 1 or D > 2048, S < 1, R neither N nor (S with N % S == 0), a null pointer.
 * AURA_E_ALIGN: a pointer not 4-byte aligned, or, when D % 4 == 0, x, table, w, b or y not 16-byte aligned.
 * N == 0 launches nothing. */
int aura_theta_gamma_norm(const float* x, const float* table, const float* w, const float* b, float eps, int64_t N,
                          int64_t S, int64_t R, int64_t D, float* y, float* mean, float* rstd, void* stream);

/* The backward.  Per token, h and n re-formed from x, the table row, mean and rstd with the forward's roundings;
 * wg = fl(w g_y), c1 = sum_d wg / D, c2 = sum_d fl(wg n) / D (row sums as above),
 *     g_h = fl(rstd * fl(fl(wg - c1) - fl(n c2))),      g_x = g_h                           written for every token.
 * Column sums over the tokens, wanted when partials / grads are given: grads [5][D] =
 *     g_w = sum g_y n,  g_b = sum g_y,  g_theta = sum g_h d_theta[row],  g_gamma = sum g_h d_gamma[row],
 *     g_amp = sum g_h d_amp[row]
 * (each product rounded, then added).  Without the derivative tables only the first two rows of grads are written.
 * The order of a token sum: G = aura_theta_gamma_groups(N) = clamp(ceil(N / 16), 1, 1024) workgroups of four waves;
 * wave v of group g adds the tokens [c (4 g + v), c (4 g + v + 1)), c = ceil(N / 4 G), in ascending order from 0; a
 * group adds its waves as ((0 + 1) + 2) + 3 and writes partials [g][5][D]; the finish launch cuts the groups into
 * eight runs of ceil(G / 8), adds each run in ascending g from 0 and the eight results in order.  A function of (N, D)
 * alone; no atomics; the same call gives the same bits.  T_N = c + 3 + ceil(G / 8) + 7 + 1.
 * partials: G * 5 * D floats of workspace (16-byte aligned when D % 4 == 0), written before they are read.
 * Errors as aura_theta_gamma_norm; AURA_E_INVAL also for one or two of the three derivative tables, partials without
 * grads or grads without partials, derivative tables without partials.  Two launches on `stream` (one without grads). */
int64_t aura_theta_gamma_groups(int64_t N);
int aura_theta_gamma_norm_backward(const float* g_y, const float* x, const float* table, const float* d_theta_or_null,
                                   const float* d_gamma_or_null, const float* d_amp_or_null, const float* mean,
                                   const float* rstd, const float* w, int64_t N, int64_t S, int64_t R, int64_t D,
                                   float* g_x, float* partials_or_null, float* grads_or_null, void* stream);

/* ---------------------------------------------------------------------------------------
 * Prosody attention
 * ------------------------------------------------------------------------------------- */

/* The attention gains that ProsodyModulatedGIF consumes, from token ids (or from three given prosody channels) in one
 * launch: prosody_channels_from_text, MultiChannelSpikingAttention.forward (src/core/language_zone/
 * multi_channel_attention.py) and the gain line of ProsodyAttentionBridge.forward (prosody_attention.py), csrc/
 * aura_prosody.hip.  Forward only: the spikes are a comparison, so the reference carries no gradient either.  All fp32,
 * every operation rounded on its own (no fused multiply-add), fl() = round to nearest even.  Per row b of B, with
 * len = clamp(lengths[b], 0, S) (S without lengths):
 *   channels  from ids (int64 or int32, 0 <= id < 2^24 so that float(id) is exact), with the accurate sinf / cosf (full
 *             range reduction: the phases reach 2e4 rad for a 65 536-word vocabulary):
 *                 amp = |sin(fl(float(id) * 0.1f))|,  pitch = |cos(fl(float(id) * 0.05f))|,
 *                 boundary = sin(fl(float(id) * 0.3f)) > 0.8f ? 1 : 0;
 *             or the three arrays amp, pitch, boundary [B][S] as given (ids NULL).
 *   LIF       per channel c with decay d = decay[c], from v = v0[b][c] (0 without v0), for t = 0 .. len - 1:
 *                 v = fl(fl(d * v) + x_t);   s_t = (v >= 1.0f);   v = fl(v - s_t)
 *             at most one spike per step; NaN and inf follow the IEEE comparison and subtraction.  v after step
 *             len - 1 is v_out[b][c] (v0 itself when len == 0).
 *   salience  sal_t = fl(fl(fl(w0 s_amp) + fl(w1 s_pitch)) + fl(w2 s_bound)),  w = weights[0 .. 2].
 *   smoothing m > 1: kw = fl(1.0f / m);  out_t = fl(kw sal[t - m/2]) + fl(kw sal[t - m/2 + 1]) + .. (m terms, added left
 *             to right from the first, sal = 0 outside [0, len)): the reference's conv1d(padding = m // 2)[:S].
 *   normalize sal_t = sal_t / fl(max_{t < len} sal + 1e-6f), a correctly rounded division.
 *   winners   the exact top k_eff = min(k, len) of sal[0 .. len): the larger value first, -0.0 and +0.0 equal, equal
 *             values to the LOWER position (torch.topk leaves this open), emitted in RANK order as int32 [B][k], the
 *             rest -1.  avg = fl(sum of the winners' values, added in rank order from the first, / float(k_eff)); 0 when
 *             len == 0.
 *   gains     mu = fl(min_gain + fl(fl(max_gain - min_gain) * tanhf(fl(gain_up * avg)))),  gains_t = fl(mu * fl(1 + sal_t)).
 *   t >= len  spikes 0, sal = 0, gains = mu.
 * decay and weights are [3] fp32 in device memory (the module's buffers) and must be finite: a NaN salience is ranked
 * as in the place code (above +inf) but is skipped by the maximum.  A row's result depends on nothing else in the
 * call: its bits are the same alone or in any batch, whatever the launch geometry.  No atomics.
 * Outputs: gains, salience [B][S], mu [B], winners [B][k], v_out [B][3]; spikes [3][B][S] and channels [3][B][S] when
 * their pointers are given.  With all five of the first group NULL and channels given, only the channels are computed
 * (ids required in practice; lengths, v0 and spikes must then be NULL, k and smoothing are ignored).
 * Against fp64 on the same fp32 phase, amp and pitch are within 2^-21 (4 ulp of a sine); tanhf is within 5 * 2^-23.
 * AURA_E_INVAL: B < 0 or B > 2^31 - 1, S < 1 or S > 8192, k < 1 or k > min(S, 256), smoothing < 1 or > 64, ids together
 *   with a channel array or neither, fewer than three channel arrays, id_bytes not 8 / 4 (ids) or 0 (channels), some but
 *   not all of the five outputs, a null decay or weights.  AURA_E_ALIGN: ids not aligned to id_bytes, any other pointer
 *   not 4-byte aligned.  B == 0 launches nothing.  One launch on `stream`. */
int aura_prosody_attention(const void* ids_or_null, int id_bytes, const float* amp, const float* pitch,
                           const float* boundary, const int32_t* lengths_or_null, const float* v0_or_null,
                           const float* decay, const float* weights, float gain_up, float min_gain, float max_gain,
                           int smoothing, int normalize, int64_t B, int64_t S, int64_t k, float* gains, float* salience,
                           float* mu, int32_t* winners, float* v_out, float* spikes_or_null, float* channels_or_null,
                           void* stream);

/* ---------------------------------------------------------------------------------------
 * Decode attention
 * ------------------------------------------------------------------------------------- */

/* One cached decoding step of HippocampalProsodyAttention (src/core/language_zone/hippocampal_attention.py): the query
 * modulation of lines 46-75, the append of the new key and value to a K/V cache, and the attention of the one new query
 * row over the positions 0 .. L, csrc/aura_decode.hip.  The module's causal forward at position L is this function of
 * the rows 0 .. L, so stepping is the same function as the forward, not an approximation.  All fp32, every operation
 * rounded on its own (no fused multiply-add), fl() = round to nearest even, expf / tanhf the accurate device functions.
 *
 * q, k_new, v_new, x [B][D], D = H dh: the three projections of the new token and the normed hidden row they were taken
 * from (x is read only with wm).  prosody [B][4] or NULL; Wp [H][4], bp [H] the prosody gate (read only with prosody);
 * wm [D], bm [1] the memory gate, both or neither (NULL: use_memory=False).  lengths int32 [B]; Kc, Vc [B][H][cap][dh].
 * Per row b and head h, L = lengths[b]:
 *   inactive  L < 0 or L >= min(cap, 256 n_chunks): nothing is written to either cache, ctx[b] = 0, scale[b][h] = 0,
 *             lengths[b] stays.  lengths[b] = -1 retires a sequence; a full cache is harmless on the device.
 *   scale     sig(a) = fl(1 / fl(1 + expf(-a)));  p = prosody[b]
 *                 g  = fl(fl(fl(fl(fl(Wp[h][0] p0) + fl(Wp[h][1] p1)) + fl(Wp[h][2] p2)) + fl(Wp[h][3] p3)) + bp[h])
 *                 sp = fl(fl(fl(1 + sig(g)) * fl(1 + fl(0.2 tanhf(p0)))) * fl(1 + fl(0.05 tanhf(p1))))     (1 without prosody)
 *                 sm = fl(1 + fl(0.5 sig(fl(dot_D(wm, x[b]) + bm[0]))))                                    (1 without wm)
 *                 s  = fl(sp * sm),   q' = fl(q * s)
 *             dot_D: lane l of a wave owns the units u = l, l + 64, .. of D / 4 (a unit is four consecutive columns) and
 *             adds fl(wm[d] x[d]) in ascending d from 0; the 64 lane sums are added by the xor butterfly 32, 16, 8, 4, 2, 1.
 *             A function of D alone.
 *   append    Kc[b][h][L] = k_new[b][h dh ..], Vc[b][h][L] = v_new[b][h dh ..], bit copies.  Position L's key and value
 *             are taken from k_new / v_new by whoever needs them, never read back from the cache.
 *   scores    z_t = fl(dot_dh(q', K_t) * isq), isq = fl(1 / sqrtf(float(dh))), t = 0 .. L.  dot_dh: G = dh / 4 units, GP the
 *             power of two >= G; unit j gives fl(fl(fl(q0 k0 + q1 k1) + q2 k2) + q3 k3) (each product rounded), the GP
 *             values (0 for j >= G) are added by the xor butterfly GP/2, .., 1.
 *   chunks    chunk c is the positions [256 c, 256 c + 256), cut by position alone.  A chunk is reduced by R = 64 / GP
 *             slots; slot r takes the positions 256 c + r + R i, i = 0, 1, .., four at a time (a block; the positions
 *             past L are left out), from (m, l, acc) = (-inf, 0, 0):
 *                 m' = max(m, z of the block);  al = (m == m') ? 1 : expf(m - m');  l = fl(l al);  acc = fl(acc al);
 *                 then for each position of the block in order: p = expf(z - m'); l = fl(l + p); acc = fl(acc + fl(p V_t)).
 *             The slots are merged by the xor butterfly GP, 2 GP, .., 32 with
 *                 M = max(m_a, m_b);  e_x = (m_x == -inf) ? 0 : expf(m_x - M);  l = fl(fl(l_a e_a) + fl(l_b e_b))  (acc alike),
 *             which is symmetric in a and b.  The chunk's (m, l, acc[dh]) goes to the workspace.
 *   merge     the second launch adds the chunks 0 .. L / 256 of a (b, h) in ascending order with the same formula
 *             (e = expf(m - M), no chunk is empty) and writes ctx[b][h dh ..] = acc / l (a correctly rounded division),
 *             the head-concatenated layout o_proj reads.  With `advance`, lengths[b] += 1 for active rows, by the second
 *             launch only: every wave of the first has read the lengths by then, and the second takes each row's chunk
 *             count from the workspace.
 * One wave per (b, h, chunk) in the first launch, four waves per workgroup, a wave whose chunk starts past L exits at
 * once; exactly one wave per (b, h) writes the append.  K and V go straight to registers in 16-byte loads.  A row's bits
 * are the same alone or in any batch, for any cap, any n_chunks >= L / 256 + 1, any other rows' lengths; two calls give
 * the same bits.  No atomics.  L = 0 gives ctx = v_new exactly (up to the sign of a zero).
 * Against fp64 on the same fp32 inputs (tests/decode_attention_rule.py derives it): with E_s the relative error of s,
 * A_t = isq sum_i |q'_i K_ti|, Dz = max_t (E_s + (log2 GP + 7) 2^-24) A_t,
 *     |ctx_d - ctx64_d| <= sum_t w_t |V_td| (expm1(2 Dz) + ((zmax - z_t) + Z) 2^-24 + 2 T 2^-24),
 *     Z = sum_t w_t (zmax - z_t),   T = 256 / R + 3 * 64 / R + 4 log2 R + 4 (L / 256 + 1) + 8.
 *
 * workspace: aura_attn_decode_workspace_bytes(B, H, dh, n_chunks) bytes, 16-byte aligned, owned by the caller, written
 * before it is read.  scale [B][H] or NULL receives s.
 * AURA_E_INVAL: B < 0, H < 1, dh % 4 != 0, dh < 4 or > 128, H dh > 2048, cap < 1 or > 32768, n_chunks < 1 or
 *   256 n_chunks > cap + 255, B H n_chunks > 2^31 - 1, a null required pointer, prosody without Wp / bp, one of wm / bm,
 *   wm without x, a workspace too small.  AURA_E_ALIGN: q, k_new, v_new, x, wm, Kc, Vc, workspace or ctx not 16-byte
 *   aligned, any other pointer not 4-byte aligned.  B == 0 launches nothing.  Two launches on `stream`. */
int64_t aura_attn_decode_workspace_bytes(int64_t B, int64_t H, int64_t dh, int64_t n_chunks);
int aura_attn_decode_step(const float* q, const float* k_new, const float* v_new, const float* x,
                          const float* prosody_or_null, const float* Wp, const float* bp, const float* wm_or_null,
                          const float* bm_or_null, int32_t* lengths, float* Kc, float* Vc, int64_t B, int64_t H,
                          int64_t dh, int64_t cap, int64_t n_chunks, int advance, float* workspace,
                          int64_t workspace_bytes, float* ctx, float* scale_or_null, void* stream);

/* Decode attention: extend.  m new tokens per row appended to a cache that already holds a context, in one pass over K
 * and V, csrc/aura_decode.hip.  Not a new formula: the rule above, once per query.
 *
 * q, k_new, v_new, x, ctx [B][m][D]; prosody [B][m][4] or NULL; scale [B][m][H] or NULL; 1 <= m <= 32; everything else as
 * in the step.  Per row b, L = lengths[b]:
 *   inactive  L < 0 or L + m > min(cap, 256 n_chunks): the row fits whole or is inactive whole.  Nothing is written to
 *             either cache, lengths[b] stays, ctx[b][j] = 0 and scale[b][j][h] = 0 for every j.
 *   active    for j = 0 .. m - 1: scale, q', scores, chunks and merge are the step's rule with L replaced by
 *             L_j = L + j and row j of q, x and prosody; query j attends the positions 0 .. L + j, whose keys and values
 *             are the cache's below L and k_new[b][t - L], v_new[b][t - L] from L on.
 *   append    Kc[b][h][L + j] = k_new[b][j][h dh ..], Vc alike, bit copies.  Positions >= L are taken from k_new /
 *             v_new by whoever needs them and never read from the cache in the launch that appends them; each is
 *             written by exactly one wave, that of the chunk (L + j) / 256.
 *   lengths   with `advance`, lengths[b] += m for active rows, by the second launch only.
 * Hence, on the same inputs, ctx[b][j], the scales, both caches and the lengths after one extend of m are bit for bit
 * what m successive calls of aura_attn_decode_step leave (step j given row j); m = 1 is the step.  The reason it holds
 * without effort: a query's operation sequence, its cut into chunks, slots and blocks by position alone and the
 * symmetric merges do not depend on what else a wave computes, and a block in which a query has no position leaves its
 * (m, l, acc) alone.
 * One wave per (b, h, chunk, group of 8 queries) in the first launch: it loads a block once and updates the running
 * states of its queries from it; a wave whose queries do not reach its chunk exits at once.  One wave per (b, j, h) in
 * the second, the chunks 0 .. (L + j) / 256 in ascending order.  No atomics; nothing depends on the batch, cap, n_chunks or the grid.
 *
 * workspace: aura_attn_decode_extend_workspace_bytes(B, m, H, dh, n_chunks) bytes (the step's for B m rows; -1 for
 * arguments the call refuses), 16-byte aligned, owned by the caller, written before it is read.
 * AURA_E_INVAL / AURA_E_ALIGN: the step's conditions, and m < 1, m > 32, B m H n_chunks > 2^31 - 1.  B == 0 launches
 * nothing.  Two launches on `stream`. */
int64_t aura_attn_decode_extend_workspace_bytes(int64_t B, int64_t m, int64_t H, int64_t dh, int64_t n_chunks);
int aura_attn_decode_extend(const float* q, const float* k_new, const float* v_new, const float* x,
                            const float* prosody_or_null, const float* Wp, const float* bp, const float* wm_or_null,
                            const float* bm_or_null, int32_t* lengths, float* Kc, float* Vc, int64_t B, int64_t m,
                            int64_t H, int64_t dh, int64_t cap, int64_t n_chunks, int advance, float* workspace,
                            int64_t workspace_bytes, float* ctx, float* scale_or_null, void* stream);

/* Decode attention: extend with per-row counts.  A restriction of the rule above to right-padded rows: row b brings only
 * its first counts[b] of the m query rows.  The arrays keep their padded shapes [B][m][..] and strides; counts int32 [B].
 * With m_b = counts[b] and L = lengths[b]:
 *   inactive  L < 0, or m_b < 0, or m_b > m, or L + m_b > min(cap, 256 n_chunks).  Nothing is written to either cache,
 *             lengths[b] stays, ctx[b][j] = 0 and scale[b][j][h] = 0 for every j < m.  The row fits by its own count:
 *             L + m_b, not L + m, so a row is active even where the padded m would not fit.
 *   m_b == 0  active but empty: nothing is written to the caches, lengths[b] stays, ctx and scale are 0.
 *   active    the queries j < m_b are the extend's rule verbatim, L_j = L + j; the positions >= L are read from the
 *             rows < m_b of k_new / v_new only.  The rows j >= m_b of q, k_new, v_new, x and prosody influence
 *             nothing (they are never loaded, so they may hold NaN) and are not appended; their ctx[b][j] and
 *             scale[b][j][h] are 0.
 *   lengths   with `advance`, lengths[b] += m_b, by the second launch only.
 * Hence, on the same inputs, row b after the call is bit for bit what m_b successive calls of aura_attn_decode_step
 * leave: ctx, the scales, both caches and the length, whatever the other rows' counts are; counts all equal to m give
 * the bits of aura_attn_decode_extend.
 * The same two kernels, compiled with the row's count in the places where m bounds the row; the instantiations behind
 * aura_attn_decode_extend are not touched.  A wave whose group of 8 queries starts at or past m_b exits at once, whole
 * and before any shuffle, so the work follows sum_b m_b, not B m.  The first launch writes a chunk count of 0 into the
 * workspace header of every query j >= m_b, and the second writes the zeros from it: it never reads a partial that
 * nobody wrote.  No atomics, no LDS, no host sync.
 *
 * workspace: aura_attn_decode_extend_workspace_bytes(B, m, H, dh, n_chunks), as above.
 * AURA_E_INVAL / AURA_E_ALIGN: the extend's conditions; counts NULL is AURA_E_INVAL, counts not 4-byte aligned
 * AURA_E_ALIGN.  B == 0 launches nothing.  Two launches on `stream`. */
int aura_attn_decode_extend_counts(const float* q, const float* k_new, const float* v_new, const float* x,
                                   const float* prosody_or_null, const float* Wp, const float* bp,
                                   const float* wm_or_null, const float* bm_or_null, int32_t* lengths,
                                   const int32_t* counts, float* Kc, float* Vc, int64_t B, int64_t m, int64_t H,
                                   int64_t dh, int64_t cap, int64_t n_chunks, int advance, float* workspace,
                                   int64_t workspace_bytes, float* ctx, float* scale_or_null, void* stream);

/* ---------------------------------------------------------------------------------------
 * Next token
 * ------------------------------------------------------------------------------------- */

/* The next token of every row of a batch from its logit row: repetition penalty, temperature, top-k, nucleus (top-p)
 * and a seeded draw, with the row's generation state kept on the device, csrc/aura_sample.hip.  What users know as the
 * tail of the reference's generate (src/core/language_zone/snn_rag_transformer.py:207-242), restated so that every
 * decision can be checked exactly.  All fp32, every operation rounded on its own, `/` a correctly rounded division,
 * expf / logf the accurate device functions.
 *
 * Per row b: logits z[0 .. V) (fp32, row b at logits + b * row_stride), seen[b][0 .. V) bytes or NULL, the row's stream
 * number (stream_ids[b], or b with stream_ids NULL).
 *   1. clean        NaN -> -inf, +inf -> FLT_MAX.  (-0 counts as +0 wherever values are ranked or returned.)
 *   2. penalty      for tokens with seen != 0, when penalty != 1:
 *                     AURA_PENALTY_DIVIDE  z / penalty for either sign (the reference generate's own line)
 *                     AURA_PENALTY_SIGNED  z < 0 ? z * penalty : z / penalty (its sampling_utils.apply_repetition_penalty)
 *                   A result of +inf is FLT_MAX again (here and in step 4); -inf stays.
 *   3. greedy       temperature == 0: the token is the argmax of the penalised z, equal z -> the lower id; no random
 *                   number is drawn, top_k and top_p are ignored, no inspection output is written.  Stop.
 *   4. temperature  z / temperature.
 *   5. top-k        1 <= top_k <= AURA_SAMPLE_MAX_K, k' = min(top_k, V): the candidates are exactly the first k' tokens
 *                   by (z descending, id ascending), in that order; rank 0 is the largest.  The reference keeps every
 *                   value that is not below the k-th (so all of its ties, in an order it leaves open); this rule keeps
 *                   exactly k', which differs from the reference only among exact ties at the threshold and keeps the
 *                   candidate set bounded.
 *   6. nucleus      e_j = expf(z_j - z_0); c_j the inclusive prefix sum of e in rank order, S = c_{k'-1}; rank j is kept
 *                   iff j == 0 or c_{j-1} <= fl(top_p * S); top_p >= 1 keeps every rank.  The sum: the ranks are cut
 *                   into blocks of 16; within a block c' runs from 0 in rank order, c' = fl(c' + e_j); the block bases
 *                   run from 0 in block order, base = fl(base + c' of the block's last rank); c_j = fl(base + c'_j).
 *                   A function of the ranks alone (not of B, the other rows or the launch), and never decreasing.
 *   7. draw         for a kept candidate with token id i: x = word 0 of Philox4x32-10, counter (i, stream,
 *                   step & 0xffffffff, step >> 32), key (seed & 0xffffffff, seed >> 32), the constants of "Replay";
 *                   u = ((x >> 9) + 0.5) * 2^-23;  d = fl(z + (-logf(-logf(u)))).  The token is the argmax of d over the
 *                   kept candidates whose z > -inf, equal d -> the lower id.  (Gumbel-max: token i with probability
 *                   softmax(z over the kept set)_i, what softmax followed by multinomial draws, with no sum and no sort
 *                   in the draw itself.)
 *   8. full vocab   top_k == 0 is allowed only with top_p >= 1: step 7 over all V tokens whose z > -inf.  top_k == 0 with
 *                   top_p < 1 is refused: a nucleus over an unbounded set needs a sorted sum over the whole vocabulary.
 *   9. empty rows   a row with no token whose z > -inf returns token -1 (n_kept = 0).
 * Row state: a row with finished[b] != 0 on entry writes pad_id, marks nothing, draws nothing and leaves its inspection
 * outputs alone.  Otherwise tokens[b * token_stride] = the token; with seen and a token >= 0, seen[b][token] = 1; with
 * finished, eos_id >= 0 and token == eos_id, finished[b] = 1.  One workgroup owns a row; its first lane writes the state
 * with plain stores after every lane has read the mask.  No global atomics.
 * Consequences: a row's token depends only on its own logits, mask, stream, seed and step; it is the same alone or in
 * any batch, with any row stride, and over repeated calls.
 *
 * Inspection outputs, each may be NULL.  With top_k >= 1: cand_ids int32 [B][k'], cand_z (the z of step 4), cand_cum
 * (c), cand_d (d; -inf for a rank that is not kept) fp32 [B][k'], n_kept int32 [B].  With top_k == 0: cand_d [B][V]
 * (-inf where z is -inf), the others are not written.
 * workspace: aura_sample_workspace_bytes(B, V, top_k, temperature) bytes (0 for greedy and for top_k == 0), 256-byte
 * aligned, owned by the caller, written before it is read.
 * AURA_E_INVAL: B < 1 or > 2^31 - 1, V < 1 or > AURA_SAMPLE_MAX_V, top_k outside [0, AURA_SAMPLE_MAX_K], top_k == 0
 *   with top_p < 1, temperature < 0 or not finite, penalty <= 0 or not finite, top_p < 0 or NaN, an unknown rule, null
 *   logits or tokens, row_stride < V, token_stride < 1, a workspace missing or too small.  AURA_E_ALIGN: tokens or
 *   stream_ids not 8-byte aligned, logits or an fp32 / int32 output not 4-byte aligned, the workspace not 256-byte
 *   aligned.  One launch on `stream`, one workgroup of 1024 lanes per row. */
#define AURA_PENALTY_DIVIDE 0
#define AURA_PENALTY_SIGNED 1
#define AURA_SAMPLE_MAX_K 1024
#define AURA_SAMPLE_MAX_V 131072
int64_t aura_sample_workspace_bytes(int64_t B, int64_t V, int64_t top_k, float temperature);
int aura_sample_next(const float* logits, int64_t row_stride, int64_t B, int64_t V, uint8_t* seen_or_null,
                     uint8_t* finished_or_null, const int64_t* stream_ids_or_null, float penalty, int penalty_rule,
                     float temperature, int64_t top_k, float top_p, uint64_t seed, uint64_t step, int64_t eos_id,
                     int64_t pad_id, int64_t* tokens, int64_t token_stride, int32_t* cand_ids, float* cand_z,
                     float* cand_cum, float* cand_d, int32_t* n_kept, void* workspace, int64_t workspace_bytes,
                     void* stream);

/* ---------------------------------------------------------------------------------------
 * Row linear
 * ------------------------------------------------------------------------------------- */

/* A linear layer for a handful of rows, with LayerNorm in front and bias, exact GELU and a residual behind, in one
 * launch, csrc/aura_rowlin.hip: what a decoding step does between its attention launches (nn.LayerNorm, nn.Linear,
 * nn.GELU and an add, each of which is a launch of its own in torch).  All fp32, fl() = round to nearest even; products
 * that feed a sum are fused (fmaf) where the rule says so and rounded on their own elsewhere; `/` and sqrtf are correctly
 * rounded, erff is the accurate device function.
 *
 * x [R][K], 1 <= R <= 32, K % 4 == 0, 4 <= K <= 8192.  One to three matrices W_j [N_j][K] (nn.Linear's layout), N_j >= 1,
 * each with a bias b_j [N_j] or NULL and an output y_j [R][N_j].  The matrices share x and the prologue; nothing
 * concatenated exists in memory.
 *   prologue  with gamma, beta [K] (K <= 2048), per row r:
 *                 sum_K(v): lane l of a wave owns the k with (k / 4) mod 64 == l and adds v_k in ascending k from 0,
 *                           s = fl(s + v_k); the 64 lane sums are added by the xor butterfly 32, 16, 8, 4, 2, 1.
 *                 mu   = fl(sum_K(x[r]) / float(K))
 *                 var  = fl(sum_K(fl(d d)) / float(K)),  d = fl(x[r][k] - mu)                     (two passes)
 *                 rstd = fl(1 / sqrtf(fl(var + eps)))          (a zero-variance row: rstd = fl(1 / sqrtf(eps)), xh = beta)
 *                 xh[r][k] = fl(fl(fl(d rstd) gamma[k]) + beta[k])
 *             Without gamma and beta, xh = x.  With xh_or_null the normalised rows are also written there, [R][K].
 *   dot       lane l of one wave chains t = fmaf(xh[r][k], W_j[n][k], t) over the k with (k / 4) mod 64 == l in
 *             ascending k, from t = 0; the 64 lane values are added by the xor butterfly 32, 16, 8, 4, 2, 1.
 *   epilogue  t = fl(dot + b_j[n]) (with a bias);  with gelu: t = fl(fl(0.5 t) fl(1 + erff(fl(t c)))), c = fl(1 / sqrt 2);
 *             with res [R][N_0] (single-matrix form only): t = fl(t + res[r][n]).  y_j[r][n] = t.
 * The order in which an element is summed is a function of K alone: not of R, N_j, the other rows, the other matrices
 * or the launch geometry.  So a row's bits are the same alone or in any batch (a NaN or inf row leaves the others
 * alone), the three-matrix form gives the bits of three single calls, and two calls give the same bits.
 * Every weight element is read from memory once per launch and serves all R rows; the x tile lives in LDS.  Workgroups
 * are independent: no atomics, no grid-wide barrier, no flag, no persistent loop; one launch is one pass.
 * `nontemporal` != 0 streams the weights with non-temporal loads (same bits; a cache policy only).
 * Against fp64 on the same fp32 inputs (tests/row_linear_rule.py derives it): with dxh the prologue's bound of
 * "Theta-gamma" (n, y) for a row sum of K,
 *     |dot - dot64| <= (K + 8) 2^-24 (sum_k |xh_k W_k| + |b|) + sum_k |W_k| dxh_k,
 * and the GELU adds 1.13 times that, 0.5 |t| (2^-19 + 5 2^-24 (1 + |t|)) and one rounding; the residual one rounding.
 *
 * AURA_E_INVAL: R < 1 or > AURA_ROW_LINEAR_MAX_ROWS, K < 4 or > AURA_ROW_LINEAR_MAX_K or K % 4 != 0, a null x, W0 or
 *   y0, N_0 < 1, a later matrix without its output or with N_j < 1 (or W2 without W1), anything of a matrix that is
 *   not given, sum N_j > 2^31 - 1, one of gamma / beta, a prologue with K > 2048 or eps < 0 or NaN, xh without a
 *   prologue, res with more than one matrix.  AURA_E_ALIGN: x, W_j, gamma, beta or xh not 16-byte aligned, any other
 *   pointer not 4-byte aligned.  One launch on `stream`. */
#define AURA_ROW_LINEAR_MAX_ROWS 32
#define AURA_ROW_LINEAR_MAX_K 8192
int aura_row_linear(const float* x, int64_t R, int64_t K, const float* W0, const float* b0_or_null, float* y0,
                    int64_t N0, const float* W1_or_null, const float* b1_or_null, float* y1_or_null, int64_t N1,
                    const float* W2_or_null, const float* b2_or_null, float* y2_or_null, int64_t N2,
                    const float* gamma_or_null, const float* beta_or_null, float eps, float* xh_or_null, int gelu,
                    const float* res_or_null, int nontemporal, void* stream);

/* Row linear: gate epilogue.  The gated memory injection of a decoding step, h + sigmoid(W_g [h; ctx] + b_g) ctx, in
 * one launch: the half of W_g that meets the memory context is folded into a per-row vector u once per generation
 * (the retrieved memories are pinned), so a step is one skinny linear layer over h with the epilogue below.
 *
 * x [R][K], one matrix W [N][.] whose rows are ldw floats apart, ldw >= K, ldw % 4 == 0 (the left [N][K] block of a
 * [N][2K] parameter is read in place: nothing is copied or concatenated), b [N] or NULL, and the per-row vectors
 * u, c, res [R][N].  No prologue, one matrix.  dot, its summation order, the limits on R and K and the
 * batch-independence property are those of "Row linear"; then
 *     t = fl(dot + b[n])                      (with a bias)
 *     a = fl(t + u[r][n])
 *     s = fl(1 / fl(1 + expf(-a)))            (expf: the device function, 1 ulp; a = -inf..: s = 0, a = +inf: s = 1)
 *     y[r][n] = fl(res[r][n] + fl(s c[r][n])) (the product is rounded on its own)
 * Against fp64 on the same fp32 inputs (tests/row_linear_epilogue_rule.py derives it), with d the dot's bound above,
 * e = 2^-24, s64 the fp64 sigmoid of the fp64 a, and every rounding of the epilogue entered at a whole ulp (2e):
 *     da = |a - a64| <= d + 2e |a|,      g = s64 (1 - s64) da exp(da),      ds = |s - s64| <= g + 6.5 e (s64 + g),
 *     |y - y64| <= |c| ds + 2e (|s64 c| + |y64|).
 *
 * AURA_E_INVAL: R, K as "Row linear"; a null x, W, u, c, res or y; N < 1 or > 2^31 - 1; ldw < K or ldw % 4 != 0.
 * AURA_E_ALIGN: x or W not 16-byte aligned, any other pointer not 4-byte aligned.  One launch on `stream`. */
int aura_row_linear_gate(const float* x, int64_t R, int64_t K, const float* W, int64_t ldw, const float* b_or_null,
                         const float* u, const float* c, const float* res, float* y, int64_t N, int nontemporal,
                         void* stream);

/* Row linear: GIF epilogue.  The current t = fl(dot + b) of a skinny linear layer (one matrix, no prologue; dot, its
 * summation order, the limits on R and K and the batch-independence property are those of "Row linear") feeds the
 * fp32 GIF step of aura_gif_run (AURA_F32; csrc/aura_gif_model.inl holds the one definition both use) bit for bit,
 * without the currents ever being written.  Every row, or token, starts from fresh state: v = 0, theta = threshold.
 *   time-invariant (time_major == 0): each of the R rows runs T steps on its own current; out is the spikes [R][T][N]:
 *       what aura_gif_run with AURA_GIF_TIME_INVARIANT makes of aura_row_linear's output.
 *   time-major (time_major != 0): R = tokens x T, R % T == 0; the rows tok T .. tok T + T - 1 are a token's T steps in
 *       order.  out [tokens][N] is the mean over T, fl(sum / float(T)) (AURA_GIF_MEAN_OUT): what aura_gif_run with
 *       AURA_GIF_MEAN_OUT makes of aura_row_linear's output viewed as [tokens][T][N].
 *       With res, m [tokens][N] and gate (one float in device memory, read by the kernel: no host read), all three
 *       or none, out is instead the hybrid mix with the residual:
 *           g = fl(1 / fl(1 + expf(-gate[0]))),   y = fl(res + fl(fl(fl(1 - g) m) + fl(g mean))).
 * 1 <= T <= 32, L >= 1.
 * AURA_E_INVAL: R, K as "Row linear"; a null x, W or out; N < 1 or > 2^31 - 1; T < 1 or > 32; L < 1; time-major with
 *   R % T != 0; one or two of res / m / gate; the mix without time_major.  AURA_E_ALIGN: x or W not 16-byte aligned,
 *   any other pointer not 4-byte aligned.  One launch on `stream`. */
int aura_row_linear_gif(const float* x, int64_t R, int64_t K, const float* W, const float* b_or_null, float* out,
                        int64_t N, int64_t T, float decay, int L, float alpha, float threshold, int time_major,
                        const float* res_or_null, const float* m_or_null, const float* gate_or_null, int nontemporal,
                        void* stream);

/* ---------------------------------------------------------------------------------------
 * Memory attend
 * ------------------------------------------------------------------------------------- */

/* The cross-attention memory injection of a decoding step, h + out_proj(softmax(q K^T / sqrt(dh)) V) with q the query
 * projection of LayerNorm(h) and K, V the projections of M memories, in one launch, csrc/aura_memattend.hip.  The
 * memories are pinned for the generation, so both D x D projections are folded, once per generation, into two tables
 * per row (the caller builds them): G[r][h][m][:] = Wq_h^T k_h[m] / sqrt(dh), s0[r][h][m] = bq_h . k_h[m] / sqrt(dh) and
 * U[r][h][m][:] = Wo[:, h] v_h[m].  All fp32, fl() = round to nearest even; `/` and sqrtf are correctly rounded, expf
 * is the device function (1 ulp).
 *
 * x [R][D], gamma, beta [D], G [R][H][M][D], s0 [R][H][M], U [R][H][M][D], bo [D] or NULL, y [R][D] (y aliases no
 * input).  1 <= R <= 32; D % 4 == 0, 4 <= D <= 2048; 1 <= M <= 32; 1 <= H M <= 1024.  Per row r:
 *   xh      the LayerNorm of "Row linear"'s prologue, bit for bit: the same row sum sum_D, mu, var (two passes), rstd and
 *           xh[k] = fl(fl(fl(d rstd) gamma[k]) + beta[k]).
 *   scores  dot(h, m): lane l of one wave chains t = fmaf(xh[k], G[r][h][m][k], t) over the k with (k / 4) mod 64 == l
 *           in ascending k, from t = 0; the 64 lane values are added by the xor butterfly 32, 16, 8, 4, 2, 1 ("Row
 *           linear"'s dot with K = D).  s[h][m] = fl(s0[r][h][m] + dot(h, m)).
 *   softmax per head: mx = max_m s[h][m] (fmaxf), e[m] = expf(fl(s[h][m] - mx)), sum = e[0] + e[1] + .. in ascending m
 *           from 0, one rounding per add, p[h][m] = fl(e[m] / sum).
 *   sum     acc[d] = 0, then acc[d] = fl(acc[d] + fl(p[h][m] U[r][h][m][d])) over (h, m) in ascending h, then ascending
 *           m: every product is rounded on its own.
 *   y[r][d] = fl(x[r][d] + fl(bo[d] + acc[d]))  (without bo: fl(x[r][d] + acc[d])).
 * The order of every sum is a function of D, H and M alone: not of R, the other rows or the launch geometry.  So a
 * row's bits are the same alone or in any batch and over repeated calls, and a NaN or inf row leaves the others alone.
 * One workgroup per row; no atomics, no flags, no host sync; one launch is one pass.
 * Against fp64 on the same fp32 inputs (tests/memory_attend_rule.py derives it), e = 2^-24, every rounding behind the dot
 * entered at a whole ulp (2e), ds the bound of "Row linear" for the score (its bias is s0), p64 the fp64 softmax:
 *     eta_m = ds_m + 2e (mx64 - s64_m + ds_m + max_k ds_k),     A_m = expm1(eta_m) + 2e exp(eta_m),
 *     B = sum_k p64_k A_k + 2e (M - 1) (1 + max_k A_k),
 *     dp_m <= p64_m (A_m (1 - p64_m) + sum_{k != m} p64_k A_k + 2e (M - 1) (1 + max_k A_k)) / (1 - B) + 2e p64_m + tiny,
 *     |y - y64| <= sum_j |U_j| dp_j + 2e H M sum_j (p64_j + dp_j) |U_j| + 2e |bo + acc64| + 2e |y64|.
 *
 * AURA_E_INVAL: R, D, H or M outside the limits above; a null x, gamma, beta, G, s0, U or y; eps < 0 or NaN.
 * AURA_E_ALIGN: x, gamma, beta, G, U, bo or y not 16-byte aligned, s0 not 4-byte aligned.  One launch on `stream`. */
#define AURA_MEMORY_ATTEND_MAX_ROWS 32
#define AURA_MEMORY_ATTEND_MAX_D 2048
#define AURA_MEMORY_ATTEND_MAX_M 32
#define AURA_MEMORY_ATTEND_MAX_HM 1024
int aura_memory_attend(const float* x, int64_t R, int64_t D, const float* gamma, const float* beta, float eps,
                       const float* G, const float* s0, const float* U, int64_t H, int64_t M,
                       const float* bo_or_null, float* y, void* stream);

/* ---------------------------------------------------------------------------------------
 * MoE zone
 * ------------------------------------------------------------------------------------- */

/* The sparse mixture of spiking experts of MoELanguageZone (src/core/language_zone/moe_language_zone.py): the liquid
 * router's top-k of E experts per token, every selected expert's SNNExpert.predict on its own tokens only, and the
 * weighted sum, in five launches, csrc/aura_moe.hip.  All fp32, unfused (-ffp-contract=off) except where fmaf is
 * written; fl() = round to nearest even; `/` is IEEE division; tanhf and expf are the device functions.  chain_K(a, w)
 * below is t = 0, then t = fmaf(a[k], w[k], t) over k in the stated order.
 *
 * Route (aura_moe_route).  x [N][Dm]; U [Hr][Dm], bU, bW [Hr] (LiquidCell.U.weight, U.bias, W.bias); gate_w [E][Hr],
 * gate_b [E]; attn_gain [N] or NULL; k = the caller's min(top_k, E).  Per row:
 *   1  g[j]  = tanhf(fl(bW[j] + fl(chain_Dm(x, U[j]) + bU[j]))), k ascending
 *   2  h[j]  = fl(dt g[j])
 *   3  z[e]  = fl(chain_Hr(h, gate_w[e]) + gate_b[e]), j ascending
 *   4  temp  = temperature, or with attn_gain fminf(fmaxf(temperature / fl(attn_gain[row] + 1e-6f), 0.1f), 5.0f);
 *      z[e]  = z[e] / temp
 *   5  mx = max_e z[e] (fmaxf), ex[e] = expf(fl(z[e] - mx)), sum = the xor butterfly 32, 16, 8, 4, 2, 1 over 64 values
 *      (ex[e] for e < E, +0 above): its order is a function of E alone.  p[e] = ex[e] / sum.
 *   6  the top k of p by (value descending, expert id ascending); NaN ranks first (then by id).  torch.topk leaves ties
 *      open; here the lower id wins.
 *   7  s = p[e_0], then s = fl(s + p[e_r]) in rank order; w[r] = p[e_r] / fl(s + 1e-8f).
 * The state of the reference's cell starts at zero, so -h_prev / (tau + 1e-6) is -0 for every finite tau > -1e-6 and
 * W.weight meets a zero vector: V and W.weight are not read.  The one case that differs from the reference's op
 * sequence: a row whose V(x) is not finite (NaN, or -inf, which makes tau NaN through softplus) beside a finite U(x)
 * gives NaN there and the finite result here.
 * Writes indices int32 [N][k], weights [N][k], probs [N][E], and into the workspace the plan: the P = N k (token, slot)
 * pairs grouped by expert, within an expert in ascending token order, cut into tiles of at most 32 pairs of one expert.
 * Places come from counts and prefix sums, never from an atomic.  Three launches.
 *
 * Experts and combine (aura_moe_experts), after aura_moe_route on the same workspace, x, indices and weights.
 * ptr_table: device array [E][4 layers + 2] of device pointers: per layer Synapsis.weight [Hh][in], Synapsis.bias [Hh],
 * GIFNeuron.linear.weight [Hh][Hh], linear.bias [Hh] (in = Dm for layer 0, Hh after), then readout.weight [Dm][Hh],
 * readout.bias [Dm]; every pointer non-null, matrices 16-byte aligned.  gif_table: device [E][layers][4] = decay, L,
 * alpha, threshold of each GIFNeuron.  Per pair (token, slot) with expert e, a = x[token]:
 *   per layer   c[n] = fl(dot_in(a, W_s[n]) + b_s[n]);  i[n] = fl(dot_Hh(c, W_g[n]) + b_g[n]);
 *               s[n] = GifModel<false>::step from v = 0, theta = threshold on i[n] (csrc/aura_gif_model.inl: the spikes
 *               of aura_gif_run at T = 1 for equal currents);  the next layer's a is s
 *   y[n] = fl(dot_Hh(s_last, W_r[n]) + b_r[n])
 *   dot_K = chain_K in this order: for each block of eight k from 0, the k's b, b + 4, b + 1, b + 5, b + 2, b + 6,
 *   b + 3, b + 7 (those below K; K % 4 == 0): a function of K alone.  It is computed as a chain of
 *   v_mfma_f32_32x32x2_f32, which is this fmaf chain bit for bit.
 * y [P][Dm] at place token k + slot; trace (or NULL: nothing written) [P][layers][Hh] receives every layer's spikes.
 *   out[token][d] = sum over the token's slots in ascending expert id of fl(w[slot] y[slot][d]), from the first
 *   product (0 + p is p): the order of the reference's loop over the experts.
 * Two launches; the expert launch is sized by the bound ceil(P / 32) + E and reads the tile count on the device.
 *
 * Properties: no global atomics, no host read; a token's indices, weights, probs, y and out are bit for bit the same
 * alone or in any batch, for any N and over repeated calls; a NaN row leaves the other rows alone.
 * Limits: 0 <= N <= AURA_MOE_MAX_N; Dm % 4 == 0, 4 <= Dm <= 256; Hh % 4 == 0, 4 <= Hh <= 512; 1 <= Hr <= 256;
 * 1 <= k <= min(E, 8); E <= 64; 1 <= layers <= 4.  GIFNeuron's L, 1 <= L <= 64, is device data in gif_table: the caller checks it.
 * AURA_E_INVAL: a size outside the limits, a null pointer other than attn_gain / trace, a workspace smaller than
 *   aura_moe_workspace_bytes(N, E, k) (which is -1 for sizes outside the limits).  AURA_E_ALIGN: x, U, y or out not
 *   16-byte aligned, the workspace not 256-byte, ptr_table not 8-byte, any other pointer not 4-byte aligned.
 *   N == 0 launches nothing. */
#define AURA_MOE_MAX_N 16777216
#define AURA_MOE_MAX_DM 256
#define AURA_MOE_MAX_HH 512
#define AURA_MOE_MAX_HR 256
#define AURA_MOE_MAX_E 64
#define AURA_MOE_MAX_K 8
#define AURA_MOE_MAX_LAYERS 4
int64_t aura_moe_workspace_bytes(int64_t N, int64_t E, int64_t k);
int aura_moe_route(const float* x, int64_t N, int64_t Dm, const float* U, const float* bU, const float* bW, int64_t Hr,
                   float dt, const float* gate_w, const float* gate_b, int64_t E, int64_t k, float temperature,
                   const float* attn_gain_or_null, int32_t* indices, float* weights, float* probs, void* workspace,
                   int64_t workspace_bytes, void* stream);
int aura_moe_experts(const float* x, int64_t N, int64_t Dm, int64_t Hh, int64_t layers, int64_t E, int64_t k,
                     const void* ptr_table, const float* gif_table, const int32_t* indices, const float* weights,
                     float* y, float* out, float* trace_or_null, const void* workspace, int64_t workspace_bytes,
                     void* stream);

/* ---------------------------------------------------------------------------------------
 * Poisson bridge
 * ------------------------------------------------------------------------------------- */

/* ContinuousToSpikeBridge with encoding 'poisson' (src/core/language_zone/spike_bridge.py), its projection, sigmoid,
 * draw, comparison and the mean over the timesteps that follows it in MoELanguageZone, in one launch,
 * csrc/aura_bridge.hip.  The reference draws torch.rand(rows, T, dim), which depends on the call's shape and on the
 * generator's history; here a draw is a function of what it belongs to, so a token's spikes are the same in a forward
 * over the sequence and in a one-token step.  All fp32, unfused (-ffp-contract=off) except where fmaf is written;
 * fl() = round to nearest even; `/` is IEEE division; expf is the accurate device function.
 *
 * THE RULE.  x [N][K]; W [H][K] (nn.Linear's layout), b [H] or NULL; T timesteps; seed; streams uint32 [B], S =
 * rows_per_stream, N = B S; start.  Row n = b S + i has stream s = streams[b] and position p = start[b] + i (start_dev,
 * int32 [B] read on the device) or start + i (the host's `start`; start_dev NULL).  For row n and channel c:
 *   1. pre-activation  z = fl(dot_K(x[n], W[c]) + b[c]), without a bias z = dot_K(x[n], W[c]); dot_K is "MoE zone"'s:
 *                      t = 0, then t = fmaf(x[k], W[k], t) over each block of eight k from 0 in the order b, b + 4,
 *                      b + 1, b + 5, b + 2, b + 6, b + 3, b + 7: a function of K alone.
 *   2. probability     q = fl(1 / fl(1 + expf(-z))).  z = +inf: q = 1; z = -inf: q = 0; NaN: NaN.
 *   3. random words    for j = 0 .. ceil(T / 4) - 1, the FOUR words w_0 .. w_3 of Philox4x32-10 with counter (c, j, p, s)
 *                      and key (seed & 0xffffffff, seed >> 32), the constants of "Replay"; word w_i serves timestep
 *                      t = 4 j + i, words with t >= T are discarded.
 *   4. uniform         u_t = ((w >> 9) + 0.5) * 2^-23, "Replay"'s: exact in fp32, never 0 or 1.
 *   5. spike           spike[n][t][c] = u_t < q ? 1 : 0.  A NaN q never spikes, q = 1 always, q = 0 never.
 *   6. rate            rate[n][c] = fl(float(count) fl(1 / float(T))), count the number of spikes over t: the sum times
 *                      the rounded reciprocal, which is how torch's device mean divides, so these are the bits of
 *                      spikes.mean(dim=1) on the GPU.  (A true division differs from it in the last bit for some
 *                      (count, T), 9 of 10 among them; torch's CPU mean is the true division.)
 * The same seed may drive "Next token": there the counter is (token id, stream, step lo, step hi) and the word decides
 * a token; here it is (channel, word group, position, stream) and the words decide spikes.  Two counters of the two
 * rules may coincide as numbers; they feed different decisions, and neither rule reads the other's words.
 *
 * Outputs: rate [N][H] always; q_or_null [N][H] the probability of step 2; spikes_or_null [N][T][H] the train.
 * Properties: no atomics, no host read, no scratch; a row's bits depend only on its own x row, stream, position and
 * seed: the same alone or in any batch, at any (S, start) split that gives the same (s, p), over repeated calls and
 * with or without the optional outputs; a NaN or inf row leaves the other rows alone.
 * Against fp64 on the same fp32 inputs (tests/poisson_bridge_rule.py derives it): with e = 2^-24,
 *     dz = |z - z64| <= (K + 8) e (sum_k |x_k W_k| + |b|),    |q - q64| <= dz / 4 + the sigmoid's own roundings.
 * Limits: 0 <= N <= AURA_BRIDGE_MAX_N; K % 4 == 0, 4 <= K <= AURA_MOE_MAX_DM; 1 <= H <= AURA_BRIDGE_MAX_H; 1 <= T <=
 * AURA_BRIDGE_MAX_T; S >= 1, N % S == 0; 0 <= start and start + S <= 2^31 (positions below 2^31); with start_dev the
 * host's start is 0 and the device positions are the caller's to keep below 2^31 (they are taken modulo 2^32 and index
 * nothing).
 * AURA_E_INVAL, nothing launched: a size outside the limits, a null x, W, streams or rate, start != 0 beside
 *   start_dev.  AURA_E_ALIGN: x or W not 16-byte aligned, any other pointer not 4-byte aligned.  N == 0 launches
 *   nothing.  One launch on `stream`: a workgroup per 32 rows and 128 channels. */
#define AURA_BRIDGE_MAX_N 16777216
#define AURA_BRIDGE_MAX_H 4096
#define AURA_BRIDGE_MAX_T 64
int aura_poisson_rate(const float* x, int64_t N, int64_t K, const float* W, const float* b_or_null, int64_t H, int64_t T,
                      uint64_t seed, const uint32_t* streams, int64_t rows_per_stream, int64_t start,
                      const int32_t* start_dev_or_null, float* rate, float* q_or_null, float* spikes_or_null,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AURA_HIP_H */
