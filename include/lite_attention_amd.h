/*
 * lite_attention_amd.h — C-ABI of the MI355X (gfx950) QK-Skip attention forward.
 *
 * This is the drop-in boundary of the hot path. It replaces, one for one, what the
 * reference reaches through `torch.ops.lite_attention.fwd`:
 *
 *   la_fwd                <- mha_fwd                hopper/_internal/cpp/flash_api.cpp:667-1249
 *                            (+ set_params_fprop    flash_api.cpp:45-163,
 *                               run_mha_fwd         flash_api.cpp:362-380,
 *                               run_flash_fwd       hopper/_internal/cpp/flash_fwd_launch_template.h:52-363)
 *   la_fwd_args           <- Flash_fwd_params + QKSkipMaskArgs
 *                                                   hopper/_internal/cpp/flash.h:12-18,48-185
 *   la_get_tile_sizes     <- tile_size_fwd_sm90     hopper/_internal/cpp/tile_size.h:10-62
 *                            (and its Python twin LiteAttention.get_MN, hopper/lite_attention.py:87-111)
 *   la_skip_list_stats    <- LiteAttention.calc_percentage   hopper/lite_attention.py:61-85
 *                            (device-side, corrected statistic)
 *   la_blockmask_to_lists <- convert_blockmask + the (missing) fwd_block entry point of the block-sparse adapter
 *                            flash_attn/flash_blocksparse_attn_interface.py:7-39,185-200: a static 0/1 block mask becomes
 *                            the read lists la_fwd walks
 *   la_combine            <- mha_combine / flash_fwd_combine (LSE-weighted merge of partial outputs,
 *                            hopper/_internal/cpp/flash_api.cpp fwd_combine; oracle
 *                            hopper/tests/test_flash_attn.py:1178-1187)
 *   la_output_error       <- nothing: the reference names "error calibration" (README.md:14) and measures no error anywhere;
 *                            one-pass fp64 error statistics of an output against a reference output, per (batch, head, row bin)
 *   la_qk_prep            <- nothing: the reference starts at the attention call; what a Wan2.x block runs on q and k just before it
 *                            (RMSNorm, 3-axis RoPE, the cast to bf16: README.md:268-323 leaves them to eager torch) in one pass
 *   la_qk_prep_fp8        <- nothing: the same pass with an e4m3 result, per-head descales and the running per-head amax a scale
 *                            is made from - the producer of the fp8 forward's operands (q, k, and v with LA_NORM_NONE)
 *   la_qk_prep_smooth     <- nothing: la_qk_prep_fp8 that can subtract a per-head vector from k before quantizing ("smooth K"), with
 *                            the deterministic column sums that vector is made from (la_colsum_finish) and the q . c row dots that
 *                            undo its shift of the LSE
 *   la_qk_prep_rows       <- nothing: the three passes above with a row map (la_qk_prep_fp8_rows, la_qk_prep_smooth_rows): out row s is
 *                            made from a row of x and rotated as a position that two int32 tables name - the token orders of
 *                            sliding-tile, radial and permuted attention, and the plain row gather that brings V and O into them
 *   la_v_colstats         <- nothing: mean and exact amax of V - mean in one read of V (with la_v_colstats_finish), for a V that is
 *                            quantized mean-shifted ("smooth V")
 *   la_attn_unshift       <- nothing: adds that mean back to the attention output (exact: the rows of P sum to 1), restores the LSE
 *                            of smoothed keys and casts, in one read of O
 *   la_v_prep_tiles       <- nothing: quantizes V as it leaves its projection straight into the V^T tiles la_fwd's e4m3 kernels stage
 *                            (with la_v_tiles_bytes / la_v_tiles_workspace_bytes), for a la_fwd under LA_FLAG_V_PREPARED: the e4m3
 *                            (B, S, Hk, D) tensor and la_fwd's own prepare pass over it drop out
 *
 * Rules of the boundary:
 *   - plain C: pointers, sizes, scalars. No torch types, no C++ types, no exceptions.
 *   - every pointer is a DEVICE pointer unless the name says `host`.
 *   - the library owns nothing, allocates nothing on the device and keeps no global mutable
 *     state (no environment variables are read either: every choice is an argument or a flag);
 *     outputs and skip lists are caller-owned. `write_list` is mutated in place.
 *   - launches are asynchronous on the given hipStream_t (passed as void*); no host sync.
 *   - return value: LA_OK (0) or a negative la_status; on error nothing has been launched.
 */
#ifndef LITE_ATTENTION_AMD_H
#define LITE_ATTENTION_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LA_ABI_VERSION 9   /* la_output_error, la_qk_prep, la_qk_prep_fp8, la_qk_prep_smooth (+ _parts, _part_rows), la_colsum_finish, la_v_colstats (+ _parts, _part_rows, _finish), la_attn_unshift, la_v_prep_tiles, la_v_tiles_bytes, la_v_tiles_workspace_bytes, la_fwd_head_thr, la_skip_list_stats_heads and la_qk_prep_rows / la_qk_prep_fp8_rows / la_qk_prep_smooth_rows were ADDED under 9: an added entry point is compatible (la_fwd_args and every older signature are unchanged), a host detects it by symbol;
                            * 9 = 8 + LA_FLAG_LIST_INT16, la_skip_list_stats_ex, la_blockmask_to_lists_ex (la_fwd_args unchanged); 8 = 7 with the sense of the two fp8 flags turned round (the reference's arithmetic is the default form of P) + LA_FLAG_HALF_VOTE + la_combine_list;
                            * 7 = 6 + la_build_info; 6 = 5 + la_blockmask_to_lists, la_device_slots (5 = 4 + skip lists and fp8 with cu_seqlens, LA_FLAG_EXACT_ROWSUM /
                            * LA_FLAG_EXACT_EXP (renamed and inverted in 8), LA_DTYPE_FP32 for la_combine); la_fwd_args unchanged since 4 */

typedef enum la_status {
    LA_OK = 0,
    LA_ERR_NULL_ARG = -1,        /* a required pointer is NULL                                   */
    LA_ERR_STRUCT_SIZE = -2,     /* args->struct_size != sizeof(la_fwd_args): ABI mismatch        */
    LA_ERR_DTYPE = -3,           /* dtype not built (flash_api.cpp:715 "only supports fp16, bf16, fp8") */
    LA_ERR_HEAD_DIM = -4,        /* head_dim not instantiated / not a multiple of 8 (flash_api.cpp:854) */
    LA_ERR_SHAPE = -5,           /* non-positive sizes, num_heads % num_heads_k != 0 (flash_api.cpp:777). seqlen_k == 0 is NOT
                                  * an error: la_fwd stores o = 0, lse = +inf like the reference (flash_api.cpp:1241-1245) */
    LA_ERR_STRIDE = -6,          /* last dim must be contiguous (flash_api.cpp:726-728) / 16-byte rows; la_fwd: a K or V row stride above
                                  * LA_MAX_KV_ROW_STRIDE_BYTES, a Q or O row stride of 2^30 elements or more */
    LA_ERR_TILE_MISMATCH = -7,   /* block_m/block_n echo != la_get_tile_sizes (list indexing would be wrong) */
    LA_ERR_LISTS = -8,           /* read list without write list, or vice versa                   */
    LA_ERR_UNSUPPORTED = -9,     /* feature outside the hot path (causal, dv != d, ...)           */
    LA_ERR_LAUNCH = -10,         /* hipLaunchKernel failed; see la_last_hip_error()               */
    LA_ERR_SEQLEN = -11,         /* sequence too long for the per-workgroup list staging in LDS, or (int16 lists) for an int16 row */
    LA_ERR_WORKSPACE = -12,      /* fp8: workspace missing or smaller than la_fwd_workspace_bytes() */
    LA_ERR_Q_WINDOW = -13        /* q_tile_begin/q_tile_count outside [0, ceil(seqlen_q/block_m)]  */
} la_status;

/* The largest K / V row stride la_fwd accepts, in BYTES. The kernels stage a 64-row key tile with one 64-bit tile address plus a per-lane
 * offset row_in_tile * row_stride_bytes + chunk + bias held in 32 bits: unsigned in the hand-scheduled bodies (rows 0 .. 63,
 * chunk + bias <= 3584: 63 * 2^26 + 3584 < 2^32), signed in the 128-row template (at most 14 rows of a wave's 16: 14 * 2^26 < 2^31).
 * 2^26 is the largest power of two inside both bounds. */
#define LA_MAX_KV_ROW_STRIDE_BYTES 67108864

/* la_fwd_args.flags */
#define LA_FLAG_KERNEL_128ROW 4u /* A/B: run the hipcc-scheduled 128-row template (32 rows per wave) where the default is the
                                  * hand-scheduled kernel: bf16 / fp16 head_dim 128 (the skip lists then use 128-row q-tiles instead of
                                  * 256-row ones: take the tile sizes from la_get_tile_sizes_ex() with the same flags) and head_dim 256
                                  * (same tiles). head_dim 96 / 192 have no such instantiation: LA_ERR_HEAD_DIM. fp8: LA_ERR_UNSUPPORTED. */
#define LA_FLAG_HALF_VOTE 64u    /* bf16 / fp16 head dims 64 / 96 / 128 - the kernels with a 256-row q-tile (no effect elsewhere; LA_FLAG_KERNEL_128ROW wins when both are set): the hand-scheduled
                                  * kernel keeps its skip lists per 128-ROW HALF of its 256-row workgroup - the reference's own q-granularity for
                                  * this head dim (kBlockM = 128, tile_size.h:35-39). la_get_tile_sizes_ex() reports (128, 64) with it. The
                                  * workgroup walks the UNION of its two halves' lists (never longer than the 256-row list of the same votes), and
                                  * the waves of a half sit out the tiles only the other half lists. Every half's output, LSE and write list are
                                  * exactly those of an independent 128-row q-tile walking its own list. At a given THRESHOLD a 128-row vote drops
                                  * more tiles than a 256-row one (13.7 % / 25 % fewer listed tiles at thr -4.22 / -2.46 on the 50-step workload).
                                  * q-tile windows: q_tile_begin even, q_tile_count even unless the window reaches the last q-tile. Lists are read
                                  * as SETS of tiles (identical to the literal walk for every well-formed list; a list with overlapping or
                                  * ascending ranges walks each named tile once). */
#define LA_FLAG_LIST_INT16 128u  /* read_list and write_list point at int16_t rows instead of int32_t ones: the same geometry [B_alloc, H, Qt, Kt+1]
                                  * contiguous and the same row format, half the bytes (the lists are the only state a caller keeps per layer: 112 -> 56 MB
                                  * at S = 75 600, H = 40; INTEGRATION.md has the table). A row is 2 * (Kt + 1) bytes and may start on any 2-byte
                                  * boundary: the kernels touch such lists with 16-bit loads and stores only. Every entry is a tile index below Kt or a
                                  * count of at most Kt, so int16 holds every well-formed list la_fwd accepts; with Kt + 1 > 32767 the flag is refused
                                  * (LA_ERR_SEQLEN) before any launch; on a launch without lists it is LA_ERR_UNSUPPORTED. must_do_list stays int32_t. Every kernel that takes lists takes both forms, and
                                  * o, lse and the written list VALUES are identical to the int32 launch's. */
#define LA_FLAG_EXACT_RESCALE 8u /* A/B: the hand-scheduled kernels rescale O on EVERY growth of a row maximum (tau = 0) instead of lazily
                                  * (bf16: only after it grew by more than 2^8; results agree to rounding, lists are identical) */
/* fp8 (e4m3) forms of P. DEFAULT = the reference's arithmetic in full: P = exp2(S c - m c + off) by the transcendental unit, rounded to e4m3 by the
 * hardware convert (softmax.h:85-87 + mainloop...:1645-1647), row sums l = sum of the UN-rounded fp32 P on the vector unit (softmax.h:275-296: LSE
 * exact to fp32). The two flags below trade that for throughput and are for callers who ask for it (round 6: until ABI 7 the encoded form was the
 * default and the reference's arithmetic behind LA_FLAG_EXACT_ROWSUM / LA_FLAG_EXACT_EXP - a drop-in's default must be the reference's results). */
#define LA_FLAG_FP8_MFMA_ROWSUM 16u /* fp8: row sums l~ = sum of the e4m3-ROUNDED P taken from the matrix pipe instead of the fp32 sum of the un-rounded P
                                  * (4-5 % faster; O = (sum P~ V) / (sum P~) is self-consistent, the LSE then carries the rounding of
                                  * P~: |LSE - exact| <= ln(1 + 2^-4), about 1e-2 on rows of a few keys, 1e-4 on long rows).
                                  * Ignored for bf16 / fp16. */
#define LA_FLAG_FP8_ENCODED_P 32u /* fp8: the BLOCK-SCALED LOG-LINEAR ENCODING of P instead of exp2 + hardware rounding (implies the matrix-pipe row sums):
                                  *  - the e4m3 byte of P is computed directly, b = sat_u8(rne(8 y + 56 - 8 delta)), y = log2 P: one FMA + one byte
                                  *    convert per score and no transcendental (the fp8 kernel is bound by vector-unit issue, not by the matrix
                                  *    pipe). Reading byte / 8 - 7 as a base-2 logarithm is the linear-mantissa exponential (1 + f for 2^f; delta =
                                  *    0.0575 centres it): per element P~ / P lies in [0.920, 1.065] (rms 3.1 %) against [0.941, 1.0625] (rms 2.65 %)
                                  *    for round-to-nearest e4m3;
                                  *  - per query row and key tile P is encoded relative to 2^t, t = floor(log2 of the row's largest P in the tile), and
                                  *    the matrix instruction multiplies by 2^t through its E8M0 block-scale operand (MX scaling of P): the 15 octaves
                                  *    of the byte grid hang below the TILE's maximum, so a diffuse tail far below the row maximum is kept with full
                                  *    relative precision (hardware rounding at the reference's offset drops P below 2^-17 of the row maximum), and
                                  *    P cannot overflow, so O is practically never rescaled.
                                  * NOT the reference's arithmetic: on the reference-generated fp8 outputs the error of O is 1.6-2.1 x that of the default
                                  * form (rms), inside the reference's own fp8 rule; |LSE - exact| <= 0.084 (rows of one or two comparable keys), about
                                  * 3e-4 of bias on long rows. +20 ... +25 % throughput at the headline shape over the default (bench.py reports all
                                  * three forms in one line). Ignored for bf16 / fp16. */
#define LA_FLAG_STATIC_SCHED 2u  /* keep one workgroup per item (static XCD map) even when a workspace is given. For
                                  * launches that must share the GPU with another kernel while they run — e.g. an RCCL
                                  * collective on another stream: persistent workgroups would hold every CU until the
                                  * launch ends, per-item workgroups release a CU every item. */
#define LA_FLAG_V_PREPARED 1u    /* fp8: `workspace` already holds the prepared V^T tiles of THIS v (an earlier
                                  * la_fwd call on the same v/workspace): skip the prepare pass. Lets a caller
                                  * split one attention into several q-tile windows (below) and pay for it once. */

typedef enum la_dtype {
    LA_DTYPE_BF16 = 0,
    LA_DTYPE_FP16 = 1,           /* q/k/v/o fp16; every path of LA_DTYPE_BF16 (lists, varlen, flags) */
    LA_DTYPE_FP8_E4M3 = 2,       /* OCP e4m3fn (gfx950), bf16 output                              */
    LA_DTYPE_FP32 = 3            /* la_combine only: fp32 result of fp32 partials                */
} la_dtype;

/*
 * Forward arguments (dense and QK-Skip launches, fixed-length and packed batches, bf16 / fp16 / fp8: every path of la_fwd). Strides are in ELEMENTS (as Flash_fwd_params, flash_api.cpp:84-103).
 * Tensors: q (B,Sq,H,D)  k (B,Sk,Hk,D)  v (B,Sk,Hk,Dv)  o (B,Sq,H,Dv)  lse (B,H,Sq) fp32 contiguous.
 * GQA / MQA: H % Hk == 0, query head h reads K/V head h / (H/Hk) (flash_api.cpp:777; the reference's
 * non-packed GQA path); fp8 descales are per (batch, K/V head) for q, k AND v (flash_api.cpp:689-691).
 *
 * Skip lists (reader/writer semantics of
 * hopper/_internal/cpp/mainloop_fwd_sm90_tma_gmma_ws.hpp:47-192):
 *   int32 [B_alloc, H, Qt, Kt+1] contiguous, Qt = ceil(Sq/block_m), Kt = ceil(Sk/block_n);
 *   row = [L, start_0, end_0, start_1, end_1, ...]; ranges descending, both ends inclusive.
 *   read_list == NULL  -> dense mode (is_skipable = false, flash_api.cpp:931-936).
 *   must_do_list: same row format, token->tile converted by the caller
 *                 (hopper/lite_attention.py:228-235); ranges are (start inclusive, end EXCLUSIVE).
 *                 must_do_is_1d != 0 -> ONE row of Kt+1 ints shared by every (b,h,q-tile)
 *                 (the reference materialises the full 4-D repeat per call, lite_attention.py:239-241).
 */
typedef struct la_fwd_args {
    uint32_t struct_size;        /* = sizeof(la_fwd_args)                                         */
    int32_t  dtype;              /* la_dtype of q,k,v                                             */

    const void* q;
    const void* k;
    const void* v;
    void*       o;               /* bf16 (also for fp8 inputs, flash_api.cpp:859)                 */
    float*      lse;             /* may be NULL: LSE not stored                                   */

    /* Elements; non-negative multiples of 16 bytes. Batch and head strides, and with them every operand's extent, are 64-bit throughout
     * (an operand may lie many GiB from its base pointer). Row strides: q / o below 2^30 elements; k / v at most
     * LA_MAX_KV_ROW_STRIDE_BYTES BYTES (2^25 bf16 / fp16 elements, 2^26 e4m3 elements) - LA_ERR_STRIDE above, before any launch. */
    int64_t q_batch_stride, q_row_stride, q_head_stride;
    int64_t k_batch_stride, k_row_stride, k_head_stride;
    int64_t v_batch_stride, v_row_stride, v_head_stride;
    int64_t o_batch_stride, o_row_stride, o_head_stride;

    int32_t batch, seqlen_q, seqlen_k;
    int32_t num_heads, num_heads_k;
    int32_t head_dim, head_dim_v;

    float   softmax_scale;       /* scores = q.k * softmax_scale (flash_api.cpp:125). 0 = uniform attention over the walked keys:
                                    O = mean of V, LSE = ln of their number (run at 2^-100 / log2 e, where every exp2 is exactly 1) */

    /* fp8 only: per-(batch, kv-head) descales, fp32; NULL = 1.0 (flash_api.cpp:1003-1022) */
    const float* q_descale; const float* k_descale; const float* v_descale;
    int64_t q_descale_batch_stride, q_descale_head_stride;
    int64_t k_descale_batch_stride, k_descale_head_stride;
    int64_t v_descale_batch_stride, v_descale_head_stride;

    const int32_t* read_list;    /* QKSkipMaskArgs::attn_read_list   flash.h:13 (int16_t rows under LA_FLAG_LIST_INT16: cast the pointer) */
    int32_t*       write_list;   /* QKSkipMaskArgs::attn_write_list  flash.h:15 (the same)        */
    const int32_t* must_do_list; /* QKSkipMaskArgs::attn_must_do_list flash.h:14; may be NULL; int32_t whatever the flags */
    int32_t        must_do_is_1d;
    float          thr;          /* QKSkipMaskArgs::thr flash.h:17 (log2 domain)                  */

    int32_t block_m, block_n;    /* echo of la_get_tile_sizes(); checked                          */

    /* Caller-owned scratch (the library allocates nothing). Size from la_fwd_workspace_bytes(); 16-byte aligned;
     * contents are scratch, valid during the call (stream-ordered).
     *   fp8: REQUIRED — the pre-transposed V tiles (64 keys x head_dim bytes per (batch, K/V head, key tile), 96 as 128; head_dim 64, 96, 128, 192, 256).
     *   bf16 / fp16: OPTIONAL, 1 KiB — eight ticket counters (one queue per XCD). With it the launch uses one
     *   persistent workgroup per CU and distributes the (batch, head, q-tile) items dynamically, which removes the
     *   cross-XCD imbalance real skip lists cause (items differ 2-3x in length; the hardware's workgroup->XCD
     *   assignment is static) and, for dense launches too since round 5 (hand-scheduled kernels; the 128-row template
     *   keeps the static map there), the per-item workgroup launch (+3.5 % at S = 75 600, +0.7 % at 16 384).
     *   Without it: one workgroup per item, static map. Results are identical. */
    void*    workspace;
    uint64_t workspace_bytes;

    /* q-tile window (ABI 3). The launch computes q-tiles [q_tile_begin, q_tile_begin + q_tile_count) of every
     * (batch, head) of the SAME problem: q/o/lse/lists are still the full tensors and are indexed by the global
     * q-tile, rows outside the window are not touched. q_tile_count == 0 means "all" (begin must then be 0).
     * Use: several launches on one stream whose outputs leave early (e.g. the head-sharded driver all-gathers
     * window i over xGMI while window i+1 computes). The reference has no equivalent (one launch per call,
     * flash_fwd_launch_template.h:359). */
    int32_t  q_tile_begin, q_tile_count;
    uint32_t flags;              /* LA_FLAG_* */
    uint32_t reserved0;          /* must be 0 */

    /* Variable-length (packed) batches (ABI 4) — the reference's cu_seqlens_q / cu_seqlens_k of mha_fwd
     * (flash_api.cpp:672-674, 736-760; Python: hopper/_internal/flash_attn_interface.py:638-682). Both NULL = fixed length.
     * Both given: q is (total_q, H, D), k/v (total_k, Hk, D), o (total_q, H, D) — the *_batch_stride fields are ignored —
     * cu_seqlens_* are DEVICE int32[batch + 1] prefix sums (sequence b = rows [cu[b], cu[b+1])), seqlen_q / seqlen_k are the
     * MAXIMUM sequence lengths (they size the grid; longer sequences are truncated to them), and lse is (H, total_q):
     * lse[h * total_q + row]. Sequences with no keys get o = 0, lse = +inf. bf16, fp16 and (round 3) fp8: the V^T prepare pass
     * reads cu_seqlens_k itself and lays every sequence's tiles on the [B, Hk, tiles of the longest sequence] grid of `workspace`.
     * One launch for the whole batch, no host sync.
     * Skip lists with cu_seqlens (round 3; the reference's varlen entry point has none): read_list / write_list / a 4-D
     * must_do_list are [>= batch, H, ceil(seqlen_q / block_m), ceil(seqlen_k / block_n) + 1] - the geometry of the MAXIMA - and
     * row (b, h, m) describes q-tile m of sequence b over that sequence's own k-tiles (tile indices relative to the sequence).
     * Rows of q-tiles past a sequence's end, and of sequences without keys, are neither read nor written. Served by the
     * hand-scheduled kernels at head_dim <= 128: with LA_FLAG_KERNEL_128ROW or a larger head_dim it is LA_ERR_UNSUPPORTED. */
    const int32_t* cu_seqlens_q;
    const int32_t* cu_seqlens_k;
    int64_t        total_q;      /* rows of q / o (= cu_seqlens_q[batch]); the head stride of lse */
} la_fwd_args;

/* Tile sizes (kBlockM, kBlockN) of the kernel that la_fwd will run for (head_dim, element size).
 * Skip-list geometry depends on them, so host code must take them from here. */
int la_get_tile_sizes(int head_dim, int element_size, int* block_m, int* block_n);
/* The same for a launch that sets `flags` (LA_FLAG_KERNEL_128ROW and LA_FLAG_HALF_VOTE change the answer). */
int la_get_tile_sizes_ex(int head_dim, int element_size, uint32_t flags, int* block_m, int* block_n);

/* Bytes of `workspace` la_fwd wants for these arguments (fp8: required; bf16 / fp16: optional, see la_fwd_args;
 * 0 under LA_FLAG_STATIC_SCHED and for dense launches of the 128-row template). Negative la_status on bad arguments. */
int64_t la_fwd_workspace_bytes(const la_fwd_args* args);

/* The forward pass. `stream` is a hipStream_t. */
int la_fwd(const la_fwd_args* args, void* stream);

/* la_fwd with one vote threshold per (batch, QUERY head) instead of the scalar args->thr (added under ABI 9: la_fwd_args is unchanged, a
 * host detects the entry by symbol). Heads are independent in attention: o, lse and the written lists of head h depend on head h's
 * threshold alone, and are bit for bit what la_fwd gives with that value as args->thr.
 *   thr_head == NULL   la_fwd(args, stream) exactly; the strides are not looked at.
 *   otherwise          the item of (b, h) votes with thr_head[b * thr_batch_stride + h * thr_head_stride] (log2 domain, as args->thr), and
 *                      args->thr is not read. thr_head is a DEVICE fp32 array owned by the caller, read by the kernels while the launch
 *                      runs (one load per work item): it may be rewritten between launches on the stream - or between replays of a
 *                      captured graph - without another host call. Strides are in ELEMENTS; thr_batch_stride = 0 gives one row for all
 *                      batches. h is the query head (the lists are per query head, also under GQA / MQA); b is the batch index, or the
 *                      sequence index of a packed batch (cu_seqlens). Every route of la_fwd with lists takes it: all kernels and dtypes,
 *                      both schedulers, q-tile windows, LA_FLAG_HALF_VOTE, LA_FLAG_LIST_INT16, LA_FLAG_V_PREPARED.
 * Special values are the scalar's: -inf flags nothing (every walked tile stays listed); NaN is the caller's error and is NOT detected.
 * Errors: every check of la_fwd, in its order and codes; then, still before any launch: a table on a dense launch (read_list == NULL)
 * LA_ERR_LISTS; a negative stride or a thr_head off a 4-byte boundary LA_ERR_STRIDE. NOT detected: a table shorter than its strides
 * and (batch, num_heads) address. */
int la_fwd_head_thr(const la_fwd_args* args, const float* thr_head, int64_t thr_batch_stride, int64_t thr_head_stride, void* stream);

/* Counts listed (= to be computed) tiles of a skip list on the device:
 *   out_counts[0] = sum over rows of sum over ranges (start - end + 1), rows = n_batch*H*Qt
 *   out_counts[1] = number of rows
 * `list` is [>=n_batch, H, Qt, Kt+1]; out_counts is a device int64[2], zeroed by the call. */
int la_skip_list_stats(const int32_t* list, int32_t n_batch, int32_t num_heads, int32_t q_tiles,
                       int32_t k_tiles, int64_t* out_counts, void* stream);

/* The same for a list of either element type: `list` holds int32_t (list_elem_size 4) or int16_t (2: the lists of a launch with
 * LA_FLAG_LIST_INT16). Other element sizes: LA_ERR_DTYPE; element size 2 with k_tiles + 1 > 32767: LA_ERR_SEQLEN. */
int la_skip_list_stats_ex(const void* list, int32_t list_elem_size, int32_t n_batch, int32_t num_heads, int32_t q_tiles,
                          int32_t k_tiles, int64_t* out_counts, void* stream);

/* The listed tiles per (batch, head): out_counts is a device int64 [n_batch, num_heads] contiguous, out_counts[b][h] = the sum over the
 * q_tiles rows of that head of sum over ranges (start - end + 1), with the row rule of la_skip_list_stats_ex (a row length below 2
 * counts as 2, one above k_tiles is clamped, a negative span counts 0). The rows per head are q_tiles for all of them. One workgroup per
 * (b, h), a fixed-order reduction: no atomics, no memset, EVERY element is written and two launches agree bit for bit. The sum over
 * (b, h) is la_skip_list_stats_ex's out_counts[0]. Errors: those of la_skip_list_stats_ex. */
int la_skip_list_stats_heads(const void* list, int32_t list_elem_size, int32_t n_batch, int32_t num_heads, int32_t q_tiles,
                             int32_t k_tiles, int64_t* out_counts, void* stream);

/* LSE-weighted merge of `num_splits` partial attention results (sequence-parallel K/V splits):
 *   o_partial   [num_splits, B, Sq, H, Dv] contiguous: fp32, or (partial_is_16bit != 0) the element type of o
 *   lse_partial fp32 [num_splits, B, H, Sq] contiguous
 *   o [B,Sq,H,Dv] contiguous of o_dtype (LA_DTYPE_BF16, LA_DTYPE_FP16, or LA_DTYPE_FP32 for fp32 partials: the reference's default there,
 *   hopper/_internal/flash_attn_interface.py:684-685), lse fp32 [B,H,Sq] (may be NULL). */
int la_combine(const void* o_partial, int32_t partial_is_16bit, const float* lse_partial,
               void* o, int32_t o_dtype, float* lse, int32_t num_splits, int32_t batch, int32_t seqlen_q,
               int32_t num_heads, int32_t head_dim_v, void* stream);

/* The same merge when the partials of the splits are SEPARATE tensors - what the calls of a split attention return, e.g. the t2t / t2v / v2t / v2v
 * calls of the reference's text + video recipe (README.md:225-246), or a ring step: stacking them into one [num_splits, ...] tensor first would
 * move every partial once more than the merge itself does. o_partials / lse_partials: HOST arrays of num_splits <= LA_COMBINE_LIST_MAX device
 * pointers, each partial [B, Sq, H, Dv] contiguous (fp32, or the element type of o when partial_is_16bit), each LSE fp32 [B, H, Sq] contiguous. */
#define LA_COMBINE_LIST_MAX 8
int la_combine_list(const void* const* o_partials, int32_t partial_is_16bit, const float* const* lse_partials,
                    void* o, int32_t o_dtype, float* lse, int32_t num_splits, int32_t batch, int32_t seqlen_q,
                    int32_t num_heads, int32_t head_dim_v, void* stream);

/* Static block mask -> read-list rows, on the device (one wave per row; no host round trip).
 *   blockmask      uint8 (0 = tile masked out, non-zero = computed), rows [q_tiles, k_tiles] contiguous; element strides between
 *                  batches and heads are arguments (0 = the same mask for every batch / head).
 *   q_tiles_valid, k_tiles_valid   device int32[batch] or NULL: the sequence of batch b has only that many q- / k-tiles (packed batches
 *                  under cu_seqlens use the mask's top-left corner): k-tiles >= k_tiles_valid[b] are dropped, rows of q-tiles >=
 *                  q_tiles_valid[b] (never read by la_fwd) get the whole corner.
 *   lists          int32 [batch, num_heads, q_tiles, k_tiles + 1] contiguous, every element written:
 *                  row = [2 * runs, start_0, end_0, ...] (descending, both ends inclusive), zero padded.
 *   empty_rows     device int32[1] or NULL: number of rows that keep no tile (row[0] = 0). Such a row has no skip-list
 *                  representation - the reader always walks its first range (mainloop_fwd_sm90_tma_gmma_ws.hpp:93-101) - the
 *                  caller decides whether to read the counter back. */
int la_blockmask_to_lists(const uint8_t* blockmask, int64_t mask_batch_stride, int64_t mask_head_stride, int32_t batch,
                          int32_t num_heads, int32_t q_tiles, int32_t k_tiles, const int32_t* q_tiles_valid,
                          const int32_t* k_tiles_valid, int32_t* lists, int32_t* empty_rows, void* stream);

/* The same with rows of either element type: `lists` is int32_t (list_elem_size 4) or int16_t (2) [batch, num_heads, q_tiles, k_tiles + 1],
 * written with element-wide stores. Other element sizes: LA_ERR_DTYPE; element size 2 with k_tiles + 1 > 32767: LA_ERR_SEQLEN. */
int la_blockmask_to_lists_ex(const uint8_t* blockmask, int64_t mask_batch_stride, int64_t mask_head_stride, int32_t batch,
                             int32_t num_heads, int32_t q_tiles, int32_t k_tiles, const int32_t* q_tiles_valid,
                             const int32_t* k_tiles_valid, void* lists, int32_t list_elem_size, int32_t* empty_rows, void* stream);

/* Error statistics of `out` against `ref`, both (B, S, H, D) with ELEMENT strides and a contiguous last dimension, each of its own
 * element type (LA_DTYPE_BF16, LA_DTYPE_FP16 or LA_DTYPE_FP32: a bf16 kernel output against the dense bf16 output, or against an fp32
 * reference). head_dim: any positive multiple of 8 (not tied to the instantiated head dims). A bin is rows_per_bin consecutive rows of
 * one (batch, head), the last one may be shorter: nbins = ceil(seqlen / rows_per_bin); rows_per_bin = seqlen gives one row of numbers
 * per head, rows_per_bin = block_m the error per q-tile.
 *   stats   device double [batch, num_heads, nbins, LA_STAT_COUNT] contiguous; EVERY element is written, the caller zeroes nothing.
 *           Per bin over all head_dim columns: the sums and the maximum below, and the number of elements at which out or ref is not
 *           finite - those elements are left out of the five other numbers (one NaN does not erase a head's statistic).
 * One pass: every element is loaded once (16-byte loads), converted to fp64 and reduced in an order the shape alone fixes - no atomics,
 * no workspace: two launches on the same data give bit-identical stats. Asynchronous on `stream`.
 * Errors (all before any HIP call): NULL out / ref / stats LA_ERR_NULL_ARG; another dtype LA_ERR_DTYPE; a non-positive size or more than
 * 2^31 - 1 bins in all LA_ERR_SHAPE; head_dim % 8 LA_ERR_HEAD_DIM; a negative stride, or a pointer / row / head (/ batch, when batch > 1)
 * stride that takes a row start off a 16-byte boundary for its dtype, LA_ERR_STRIDE. */
typedef enum la_error_stat {
    LA_STAT_ABS_DIFF = 0,        /* sum |out - ref|      */
    LA_STAT_ABS_REF = 1,         /* sum |ref|            */
    LA_STAT_SQ_DIFF = 2,         /* sum (out - ref)^2    */
    LA_STAT_SQ_REF = 3,          /* sum ref^2            */
    LA_STAT_MAX_ABS_DIFF = 4,    /* max |out - ref|      */
    LA_STAT_NONFINITE = 5        /* elements where out or ref is NaN or +-inf */
} la_error_stat;
#define LA_STAT_COUNT 6
int la_output_error(const void* out, int32_t out_dtype, int64_t out_batch_stride, int64_t out_row_stride, int64_t out_head_stride,
                    const void* ref, int32_t ref_dtype, int64_t ref_batch_stride, int64_t ref_row_stride, int64_t ref_head_stride,
                    int32_t batch, int32_t seqlen, int32_t num_heads, int32_t head_dim, int32_t rows_per_bin,
                    double* stats, void* stream);

/* The q / k prologue of a Wan2.x-style attention block in one pass: RMSNorm, 3-axis RoPE on INTERLEAVED pairs, the cast to bf16 / fp16.
 * Per token (b, s) of x (B, S, H, D), in fp32 with ONE rounding at the store:
 *   r       = rsqrt(mean(x^2 over the norm group) + eps)     LA_NORM_TOKEN: the H*D elements of the token (Wan's RMSNorm(dim));
 *                                                            LA_NORM_HEAD: the D elements of one head; LA_NORM_NONE: r = 1, weight ignored
 *   y[h][c] = x[h][c] * r * w[c']                            w fp32 [H*D] (TOKEN) or [D] (HEAD); weight == NULL reads as ones
 *   p = pos_offset + s;  (c0, c1, c2) = (p / (e1*e2), (p / e2) % e1, p % e2)     for axis_extent = (e0, e1, e2)
 *   pair j of a head = elements (2j, 2j+1); axis a owns pairs [P_a, P_a + n_a), P_a = n_0 + ... + n_(a-1), n = axis_pairs
 *   (cos, sin) = rope_table[a][c_a][j - P_a]                 fp32 [e_a, n_a, 2] contiguous, built on the host: no transcendental on the device
 *   out(2j) = y(2j) cos - y(2j+1) sin;  out(2j+1) = y(2j) sin + y(2j+1) cos;  pairs j >= n_0 + n_1 + n_2 pass through (partial rotary)
 *   all three tables NULL: no rotation (norm and cast only, e.g. the q / k of a cross-attention)
 * Arithmetic: the sum of squares is fp32, like the torch expression it replaces - a token whose squares overflow fp32 gives what torch
 * gives (r = 0). Against Wan's `.type_as(x) * weight` followed by a rope that rounds again this has one fewer intermediate rounding.
 * The order of the reduction depends on the shape alone: two launches give bit-identical output. Asynchronous on `stream`; no workspace,
 * no atomics. x is read once and out written once, 16 bytes at a time.
 * In-place (out == x) is allowed when the two dtypes have equal size and all strides are equal: a token's elements are all read before
 * any of them is stored (LA_NORM_HEAD / LA_NORM_NONE: a head's elements). ANY OTHER overlap of x and out is the caller's error and is
 * not detected.
 * Errors (all before any HIP call): NULL args / x / out LA_ERR_NULL_ARG; struct_size LA_ERR_STRUCT_SIZE; in_dtype other than bf16 / fp16 /
 * fp32 or out_dtype other than bf16 / fp16 LA_ERR_DTYPE; an unknown norm_mode LA_ERR_UNSUPPORTED; a non-positive size LA_ERR_SHAPE;
 * head_dim % 8 != 0 or head_dim > 256 LA_ERR_HEAD_DIM; LA_NORM_TOKEN with H*D > 16384 LA_ERR_UNSUPPORTED (the token stays in
 * registers between the reduction and the store: those of one wave up to H*D = 5120, of the four waves of a workgroup up to 16384 = 256
 * lanes x 64 elements); a negative stride, a pointer or a used stride (batch / row / head, one whose dimension is larger than 1) that takes
 * a row start off a 16-byte boundary for its dtype, a head stride of 2^31 / H elements or more, a weight off 16 bytes or a table off 8
 * bytes LA_ERR_STRIDE; a negative axis_pairs entry or their sum above head_dim / 2 LA_ERR_SHAPE; a NULL table with axis_pairs > 0
 * unless all three are NULL LA_ERR_NULL_ARG; pos_offset < 0, or, when rotating, a non-positive extent or pos_offset + seqlen > e0*e1*e2
 * LA_ERR_SHAPE. */
typedef enum la_norm_mode {
    LA_NORM_NONE = 0,
    LA_NORM_TOKEN = 1,
    LA_NORM_HEAD = 2
} la_norm_mode;
typedef struct la_qk_prep_args {
    uint32_t struct_size;        /* = sizeof(la_qk_prep_args)                                     */
    int32_t  in_dtype;           /* la_dtype of x: LA_DTYPE_BF16, LA_DTYPE_FP16 or LA_DTYPE_FP32  */
    int32_t  out_dtype;          /* la_dtype of out: LA_DTYPE_BF16 or LA_DTYPE_FP16               */
    int32_t  norm_mode;          /* la_norm_mode                                                  */
    const void* x;               /* (B, S, H, D), last dimension contiguous                       */
    void*       out;             /* (B, S, H, D), last dimension contiguous                       */
    int64_t x_batch_stride, x_row_stride, x_head_stride;          /* in elements                  */
    int64_t out_batch_stride, out_row_stride, out_head_stride;
    int32_t batch, seqlen, num_heads, head_dim;
    const float* weight;         /* fp32 [H*D] (LA_NORM_TOKEN) or [D] (LA_NORM_HEAD); NULL = ones  */
    float   eps;
    int32_t pos_offset;          /* position of row 0 on the (e0, e1, e2) grid, row-major         */
    const float* rope_table[3];  /* fp32 [axis_extent[a], axis_pairs[a], 2] = (cos, sin)           */
    int32_t axis_extent[3];
    int32_t axis_pairs[3];
} la_qk_prep_args;
int la_qk_prep(const la_qk_prep_args* args, void* stream);

/* la_qk_prep with an e4m3 (OCP e4m3fn, LA_DTYPE_FP8_E4M3) result and the per-head scales the fp8 la_fwd takes: the producer of its
 * operands. Nothing is quantized inside la_fwd; the caller owns the scales and hands la_fwd the SAME descale tensors it gave here.
 * With y the fp32 value la_qk_prep would round (same norm, weight and rope, in the same order) and g = h / heads_per_scale:
 *   amax[b][g]  = max(amax[b][g], |y|)   over the unscaled y. A RUNNING maximum into the caller's fp32 buffer (zero it for a fresh one),
 *                 taken as the unsigned maximum of the bit pattern of |y|: independent of the order (two launches agree bitwise), and
 *                 a NaN anywhere in the group makes amax[b][g] NaN. One global atomic per (group, batch) and workgroup.
 *   out         = e4m3_rne(clamp(y * (1 / descale[b][g]), -448, +448))   round to nearest even; the clamp is explicit (no mode bit
 *                 matters) and keeps a NaN a NaN; descale == NULL reads as 1.0; the reciprocal is one IEEE division per group. The
 *                 cast is torch's float8_e4m3fn cast.
 *   out == NULL   the amax pass alone: x is read once, nothing but amax is written. Amax pass + quantizing pass = exact "current
 *                 scaling" in two reads and one 1-byte write; with the previous step's amax ("delayed scaling") one read, one write.
 * heads_per_scale: 1 for k and v, H_q / H_kv for q - la_fwd's q / k / v descales are per (batch, kv-head). LA_NORM_NONE without tables
 * is the V form (scale, clamp, cast, amax). descale and amax are fp32 [batch, num_heads / heads_per_scale] addressed by their strides
 * (in elements). A descale that is zero, negative or not finite is the caller's error and is NOT detected.
 * out must not overlap x (the element sizes differ: there is no in-place form); an overlap is the caller's error and is not detected.
 * Errors (all before any HIP call), in the codes of la_qk_prep: NULL args / x, or out and amax both NULL, LA_ERR_NULL_ARG; in_dtype
 * LA_ERR_DTYPE; heads_per_scale < 1 or not a divisor of num_heads LA_ERR_SHAPE; a negative descale / amax stride, or one of the two
 * pointers off a 4-byte boundary, LA_ERR_STRIDE; more than 1024 heads LA_ERR_UNSUPPORTED (a workgroup keeps the scale and the running
 * maximum of every head in LDS); an out pointer or used out stride that takes a row, head or batch start off an 8-byte boundary
 * LA_ERR_STRIDE; everything else (norm_mode, sizes, head_dim, the x alignment rules, weight, tables, positions) as la_qk_prep. */
typedef struct la_qk_prep_fp8_args {
    uint32_t struct_size;        /* = sizeof(la_qk_prep_fp8_args)                                 */
    int32_t  in_dtype;           /* la_dtype of x: LA_DTYPE_BF16, LA_DTYPE_FP16 or LA_DTYPE_FP32  */
    int32_t  norm_mode;          /* la_norm_mode                                                  */
    int32_t  heads_per_scale;    /* heads that share one descale / amax element; divides num_heads */
    const void* x;               /* (B, S, H, D), last dimension contiguous                       */
    void*       out;             /* e4m3 (B, S, H, D), last dimension contiguous; NULL: amax only */
    int64_t x_batch_stride, x_row_stride, x_head_stride;          /* in elements                  */
    int64_t out_batch_stride, out_row_stride, out_head_stride;
    int32_t batch, seqlen, num_heads, head_dim;
    const float* weight;         /* fp32 [H*D] (LA_NORM_TOKEN) or [D] (LA_NORM_HEAD); NULL = ones  */
    float   eps;
    int32_t pos_offset;          /* position of row 0 on the (e0, e1, e2) grid, row-major         */
    const float* rope_table[3];  /* fp32 [axis_extent[a], axis_pairs[a], 2] = (cos, sin)           */
    int32_t axis_extent[3];
    int32_t axis_pairs[3];
    const float* descale;        /* fp32 [B, H / heads_per_scale] by the strides below; NULL = 1.0 */
    int64_t descale_batch_stride, descale_head_stride;
    float*  amax;                /* fp32 [B, H / heads_per_scale]; NULL = not wanted (then out must be given) */
    int64_t amax_batch_stride, amax_head_stride;
} la_qk_prep_fp8_args;
int la_qk_prep_fp8(const la_qk_prep_fp8_args* args, void* stream);

/* la_qk_prep_fp8 with K smoothing: the same pass can subtract a per-head vector before it quantizes, and collect what a caller needs
 * to choose that vector and to undo its effect on the LSE. Subtracting c[b][h][:] from every key of a head lowers every score of a
 * query row by the same softmax_scale * (q . c): P, O and the skip vote are unchanged, LSE' = LSE - softmax_scale * (q . c) (natural
 * log). With y the fp32 value la_qk_prep would round (same norm, weight and rope, in the same order); every addition is optional:
 *   shift        fp32 [B, H, D] by its strides (elements). y' = y - shift[b][h][:], ONE fp32 subtraction behind the rope and before
 *                scale and clamp; amax becomes the running maximum of |y'| and out = e4m3_rne(clamp(y' * (1 / descale))). NULL: y' = y.
 *   colsum_part  fp32 [n_parts, B, H, D] contiguous, n_parts = la_qk_prep_smooth_parts(S, H, D): part[p][b][h][d] = the sum of the
 *                UNSHIFTED y over rows [p R, (p + 1) R) of the batch, R = la_qk_prep_smooth_part_rows(S, H, D), added in row order from
 *                0.0f (a part without rows is written as zeros; every element is written). The row -> part map and the order of the
 *                additions depend on (S, H, D) alone - not on the device, the grid or the timing; no float atomics: two launches
 *                agree bitwise, and a launch that also quantizes reports the same sums as one that does not.
 *   dot_vec / dot_out   dot_vec fp32 [B, H / heads_per_dot, D] by its strides, dot_out fp32 [B, H, S] contiguous (the layout of lse):
 *                dot_out[b][h][s] = sum_d y[b][s][h][d] * dot_vec[b][h / heads_per_dot][d], of the UNSHIFTED, unquantized y, in a fixed
 *                order (bit-reproducible). For q: heads_per_dot = H_q / H_kv and dot_vec = the shift given for k. Both or neither.
 *   out == NULL  nothing is quantized (a sums-only, dots-only or amax-only pass); allowed when amax, colsum_part or dot_out is given.
 * la_colsum_finish: mean_out[b][h][d] = (part[0][b][h][d] + part[1][b][h][d] + ...) / S, added in index order; mean_out by its strides.
 * With shift, colsum_part and dot_vec all NULL the call IS la_qk_prep_fp8 (the same kernels, the same bits).
 * Errors (all before any HIP call), in this order: NULL args LA_ERR_NULL_ARG; struct_size LA_ERR_STRUCT_SIZE; NULL x, or out, amax,
 * colsum_part and dot_out all NULL, or exactly one of dot_vec / dot_out, LA_ERR_NULL_ARG; in_dtype LA_ERR_DTYPE; heads_per_scale, or
 * (with dot_vec) heads_per_dot, below 1 or not a divisor of num_heads LA_ERR_SHAPE; a negative descale / amax stride, or descale, amax
 * or dot_out off a 4-byte boundary, LA_ERR_STRIDE; a negative shift / dot_vec stride, shift, dot_vec or colsum_part off a 16-byte
 * boundary, or a used shift / dot_vec stride (batch > 1; more than one head / group) that is no multiple of 4 elements LA_ERR_STRIDE;
 * then every check of la_qk_prep_fp8 from norm_mode on, in its order and codes; more than 1024 heads LA_ERR_UNSUPPORTED; colsum_part
 * with more column sums than a thread keeps in LDS LA_ERR_UNSUPPORTED: LA_NORM_TOKEN serves every H*D it accepts, LA_NORM_HEAD /
 * LA_NORM_NONE serve H <= 16 * (64 / G) heads, G = D / 8 rounded up to a power of two (64 heads of 128, 32 of 256).
 * NOT detected: a colsum_part shorter than n_parts * B * H * D, a dot_out shorter than B * H * S, buffers that overlap each other, x or
 * out, a descale that is zero, negative or not finite. */
typedef struct la_qk_prep_smooth_args {
    uint32_t struct_size;        /* = sizeof(la_qk_prep_smooth_args)                              */
    int32_t  in_dtype;           /* la_dtype of x: LA_DTYPE_BF16, LA_DTYPE_FP16 or LA_DTYPE_FP32  */
    int32_t  norm_mode;          /* la_norm_mode                                                  */
    int32_t  heads_per_scale;    /* heads that share one descale / amax element; divides num_heads */
    const void* x;               /* (B, S, H, D), last dimension contiguous                       */
    void*       out;             /* e4m3 (B, S, H, D), last dimension contiguous; NULL: not stored */
    int64_t x_batch_stride, x_row_stride, x_head_stride;          /* in elements                  */
    int64_t out_batch_stride, out_row_stride, out_head_stride;
    int32_t batch, seqlen, num_heads, head_dim;
    const float* weight;         /* fp32 [H*D] (LA_NORM_TOKEN) or [D] (LA_NORM_HEAD); NULL = ones  */
    float   eps;
    int32_t pos_offset;          /* position of row 0 on the (e0, e1, e2) grid, row-major         */
    const float* rope_table[3];  /* fp32 [axis_extent[a], axis_pairs[a], 2] = (cos, sin)           */
    int32_t axis_extent[3];
    int32_t axis_pairs[3];
    const float* descale;        /* fp32 [B, H / heads_per_scale] by the strides below; NULL = 1.0 */
    int64_t descale_batch_stride, descale_head_stride;
    float*  amax;                /* fp32 [B, H / heads_per_scale]; NULL = not wanted               */
    int64_t amax_batch_stride, amax_head_stride;
    const float* shift;          /* fp32 [B, H, D] by the strides below; NULL = no shift           */
    int64_t shift_batch_stride, shift_head_stride;
    float*  colsum_part;         /* fp32 [n_parts, B, H, D] contiguous; NULL = not wanted          */
    const float* dot_vec;        /* fp32 [B, H / heads_per_dot, D] by the strides below; NULL = no dots */
    int64_t dot_vec_batch_stride, dot_vec_head_stride;
    float*  dot_out;             /* fp32 [B, H, S] contiguous; given exactly when dot_vec is       */
    int32_t heads_per_dot;       /* heads that share one dot_vec row; divides num_heads            */
    int32_t reserved0;           /* 0                                                              */
} la_qk_prep_smooth_args;
int la_qk_prep_smooth(const la_qk_prep_smooth_args* args, void* stream);
/* Parts and rows per part of colsum_part for a shape: pure functions of their arguments (LA_ERR_SHAPE for a non-positive one). */
int la_qk_prep_smooth_parts(int32_t seqlen, int32_t num_heads, int32_t head_dim);
int la_qk_prep_smooth_part_rows(int32_t seqlen, int32_t num_heads, int32_t head_dim);
/* Errors: NULL part / mean_out LA_ERR_NULL_ARG; a non-positive size LA_ERR_SHAPE; a negative stride or a pointer off 4 bytes LA_ERR_STRIDE. */
int la_colsum_finish(const float* part, int32_t n_parts, int32_t batch, int32_t num_heads, int32_t head_dim, int32_t seqlen,
                     float* mean_out, int64_t mean_batch_stride, int64_t mean_head_stride, void* stream);

/* Token orders: la_qk_prep, la_qk_prep_fp8 and la_qk_prep_smooth with a ROW MAP (added under ABI 9: the three argument structs are
 * unchanged, a host detects the entry points by symbol). Non-causal attention is permutation-equivariant over tokens, so a caller may
 * run it in any token order - bricks of the (frame, height, width) grid, zig-zag ring shards, a pruned sequence, several clips - when
 * every row is still rotated as the position it HAS. out has args->seqlen rows, x has src_seqlen rows; for out row s of batch b, with
 * i = b * batch_stride + s:
 *   src = src_rows ? src_rows[i] : s                      the row of x that is read; the result is stored to row s of out
 *   p   = pos_offset + (positions ? positions[i] : src)   the rope position of the row (la_qk_prep: p = pos_offset + s)
 * Everything behind the load is la_qk_prep's / la_qk_prep_fp8's / la_qk_prep_smooth's own arithmetic in its own order: a row's bits
 * depend on the row it is made from and on its position alone. amax is order-free; colsum_part sums the rows of each part in the order
 * of the OUT rows (the parts are cut from args->seqlen); dot_out is indexed by the out row. The wave that owns a token reads its two
 * table entries in front of the token: no extra pass, no workspace, no atomics beyond those of the unmapped forms.
 * The kernels CLAMP what they read from the tables, src into [0, src_seqlen) and p into [0, e0*e1*e2), before use: an entry outside
 * its range reads the nearest row of x or of the rope tables, never memory outside them. This is the definition of such an entry, not
 * an error path; a host that wants it reported checks its table once, when it builds it.
 * LA_NORM_NONE without rope tables and with src_rows is a plain row gather (16-bit to the same 16-bit type: an exact copy of finite
 * values), which is how V, hidden states and O are brought into and out of an order.
 * A map with both tables NULL and src_seqlen == args->seqlen IS the unmapped entry point: the same kernels, the same bits.
 * Errors (all before any HIP call): the checks of the unmapped entry point in its order and codes, and with them: NULL map
 * LA_ERR_NULL_ARG (with NULL args); map->struct_size LA_ERR_STRUCT_SIZE (behind args->struct_size); src_seqlen < 1, or src_rows NULL
 * and src_seqlen < seqlen, LA_ERR_SHAPE (with the sizes); x's row stride is a used stride when src_seqlen > 1; src_rows or positions
 * off a 4-byte boundary or a negative batch_stride LA_ERR_STRIDE (behind the strides of x and out); src_rows with out == x
 * LA_ERR_UNSUPPORTED (a gather in place is not defined); when rotating, positions == NULL holds pos_offset + src_seqlen to e0*e1*e2
 * (LA_ERR_SHAPE) and positions != NULL holds nothing (the clamp). NOT detected: a table shorter than [B or 1][seqlen]. */
typedef struct la_row_map {
    uint32_t struct_size;        /* = sizeof(la_row_map)                                          */
    int32_t  src_seqlen;         /* rows of x (out has args->seqlen rows)                         */
    const int32_t* src_rows;     /* [B or 1][seqlen]; NULL: s                                     */
    const int32_t* positions;    /* [B or 1][seqlen]; NULL: the source row index                  */
    int64_t  batch_stride;       /* elements; 0: one map for all batches                          */
} la_row_map;
int la_qk_prep_rows(const la_qk_prep_args* args, const la_row_map* map, void* stream);
int la_qk_prep_fp8_rows(const la_qk_prep_fp8_args* args, const la_row_map* map, void* stream);
int la_qk_prep_smooth_rows(const la_qk_prep_smooth_args* args, const la_row_map* map, void* stream);

/* V smoothing: the twin of K smoothing for the one operand that is quantized as it leaves its projection. la_fwd divides by its own
 * row sum, so the rows of P sum to 1 over whatever keys a row visits - with skip lists, with split keys and after an LSE merge - and
 *   P (V - 1 m^T) + 1 m^T = P V     for any vector m[b][h_kv][:].
 * V is quantized as V - m (la_qk_prep_smooth with LA_NORM_NONE, shift = m, descale), la_fwd runs unchanged on the shifted codes, and
 * la_attn_unshift adds m to O in fp32: the rounding of V and of the e4m3 P is paid on the centred values only.
 *
 * la_v_colstats: x (B, S, H, D) bf16 / fp16 / fp32 by its strides (elements), last dimension contiguous, head_dim % 8 == 0 and <= 256;
 * no norm, no rope, no weight. stat_part fp32 [n_parts, 3, B, H, D] contiguous: stat_part[p][0 / 1 / 2][b][h][d] = the SUM, MINIMUM and
 * MAXIMUM of float(x[b][s][h][d]) over rows s in [p R, (p + 1) R), n_parts = la_v_colstats_parts(S, H, D), R =
 * la_v_colstats_part_rows(S, H, D) = max(16, ceil(S * (H * D / 8) / 131072)): pure functions of (S, H, D), not of the device, the grid
 * or the timing. The sum is added in row order from 0.0f; no float atomics: two launches agree bit for bit. A part without rows is
 * written as 0, +inf, -inf; every element is written. A NaN in a column makes that column's sum NaN; minimum and maximum skip it.
 * One read of x.
 * la_v_colstats_finish: mean_out[b][h][d] = (sum_0 + sum_1 + ...) / S, added in index order; amax_out[b][h] = max over d of
 * max(|fl(vmax - mean)|, |fl(mean - vmin)|), one fp32 subtraction each, taken as the unsigned maximum of the bit patterns (a NaN mean
 * makes that head's amax NaN and no other's). Rounding is monotone, so this is the largest |fl(x - mean)| over the rows: the bits
 * la_qk_prep_smooth reports with shift = mean_out, LA_NORM_NONE, a zeroed amax and out = NULL - mean and exact amax for one read of x
 * instead of two. amax_out is WRITTEN, not accumulated; NULL: not wanted. mean_out fp32 [B, H, D] and amax_out fp32 [B, H] by their
 * strides (elements); n_parts / batch / num_heads / head_dim describe stat_part.
 * Errors of la_v_colstats (all before any HIP call), in this order: NULL args LA_ERR_NULL_ARG; struct_size LA_ERR_STRUCT_SIZE; NULL x or
 * stat_part LA_ERR_NULL_ARG; in_dtype LA_ERR_DTYPE; a non-positive size LA_ERR_SHAPE; head_dim % 8 != 0 or above 256 LA_ERR_HEAD_DIM; a
 * negative stride, x or stat_part off a 16-byte boundary, or a used x stride (seqlen > 1: row, num_heads > 1: head, batch > 1: batch)
 * that takes a row, head or batch start off one, LA_ERR_STRIDE. Of la_v_colstats_finish: NULL part / mean_out LA_ERR_NULL_ARG; a
 * non-positive size LA_ERR_SHAPE; head_dim above 256 LA_ERR_HEAD_DIM; a negative stride or a pointer off 4 bytes LA_ERR_STRIDE.
 * NOT detected: a stat_part shorter than n_parts * 3 * B * H * D floats, buffers that overlap. */
typedef struct la_v_colstats_args {
    uint32_t struct_size;        /* = sizeof(la_v_colstats_args)                                  */
    int32_t  in_dtype;           /* la_dtype of x: LA_DTYPE_BF16, LA_DTYPE_FP16 or LA_DTYPE_FP32  */
    const void* x;               /* (B, S, H, D), last dimension contiguous                       */
    float*      stat_part;       /* fp32 [n_parts, 3, B, H, D] contiguous                         */
    int64_t x_batch_stride, x_row_stride, x_head_stride;          /* in elements                  */
    int32_t batch, seqlen, num_heads, head_dim;
} la_v_colstats_args;
int la_v_colstats(const la_v_colstats_args* args, void* stream);
/* Parts and rows per part of stat_part for a shape: pure functions of their arguments (LA_ERR_SHAPE for a non-positive one). */
int la_v_colstats_parts(int32_t seqlen, int32_t num_heads, int32_t head_dim);
int la_v_colstats_part_rows(int32_t seqlen, int32_t num_heads, int32_t head_dim);
int la_v_colstats_finish(const float* part, int32_t n_parts, int32_t batch, int32_t num_heads, int32_t head_dim, int32_t seqlen,
                         float* mean_out, int64_t mean_batch_stride, int64_t mean_head_stride,
                         float* amax_out, int64_t amax_batch_stride, int64_t amax_head_stride, void* stream);

/* la_attn_unshift: the restoring pass, one read of the attention output.
 *   out[b][s][h][:]  = round_to_out_dtype(float(o[b][s][h][:]) + shift[b][h / heads_per_vec][:])     one fp32 addition, one rounding
 *   lse_out[b][h][s] = fmaf(softmax_scale, lse_dot[b][h][s], lse[b][h][s])                            only when lse_dot is given
 * o bf16 / fp16 (B, S, H, D) by its strides - what la_fwd returns; out bf16, fp16 or fp32 by its OWN strides (e.g. the (B, S, H * D)
 * fp32 tensor an output projection reads). out may BE o (equal element sizes and strides: a chunk of 8 elements is read completely
 * before it is written, by the one thread that touches it); any other overlap of the two is NOT detected. shift fp32 [B, H_kv, D] by
 * its strides, heads_per_vec = H_q / H_kv (GQA / MQA); NULL: nothing is added (a cast / LSE pass). lse, lse_dot, lse_out fp32 [B, H, S]
 * contiguous (the layout of la_fwd's lse):
 *   lse       optional. When given, a row whose lse is +inf or -inf is written as ZEROS and its lse_out is its lse: la_fwd's empty sum
 *             (seqlen_k == 0 gives O = 0, LSE = +inf; an empty partial -inf) - no weights carry the shift. A NaN lse takes the normal path.
 *   lse_dot / lse_out   both or neither, and only with lse: la_qk_prep_smooth's q . c row dots and the LSE of the unshifted keys (K
 *             smoothing undone in the same pass). lse_out may be lse (an element is read and written by one thread).
 * Errors (all before any HIP call), in this order: NULL args LA_ERR_NULL_ARG; struct_size LA_ERR_STRUCT_SIZE; NULL o or out, exactly one
 * of lse_dot / lse_out, or the two without lse, LA_ERR_NULL_ARG; o_dtype not bf16 / fp16 or out_dtype not bf16 / fp16 / fp32
 * LA_ERR_DTYPE; a non-positive size, or (with shift) heads_per_vec below 1 or not a divisor of num_heads, LA_ERR_SHAPE; head_dim % 8 != 0
 * LA_ERR_HEAD_DIM; a negative stride, o, out or shift off a 16-byte boundary, a used stride of them that takes a row, head or batch
 * start off one, or lse / lse_dot / lse_out off a 4-byte boundary, LA_ERR_STRIDE. */
typedef struct la_attn_unshift_args {
    uint32_t struct_size;        /* = sizeof(la_attn_unshift_args)                                */
    int32_t  o_dtype;            /* la_dtype of o: LA_DTYPE_BF16 or LA_DTYPE_FP16                 */
    int32_t  out_dtype;          /* la_dtype of out: LA_DTYPE_BF16, LA_DTYPE_FP16 or LA_DTYPE_FP32 */
    int32_t  heads_per_vec;      /* query heads that share one shift row: H_q / H_kv              */
    const void* o;               /* (B, S, H, D), last dimension contiguous                       */
    void*       out;             /* (B, S, H, D) by its own strides; may be o                     */
    int64_t o_batch_stride, o_row_stride, o_head_stride;          /* in elements                  */
    int64_t out_batch_stride, out_row_stride, out_head_stride;
    int32_t batch, seqlen, num_heads, head_dim;
    const float* shift;          /* fp32 [B, H / heads_per_vec, D] by the strides below; NULL = no shift */
    int64_t shift_batch_stride, shift_head_stride;
    const float* lse;            /* fp32 [B, H, S] contiguous; NULL = no empty-row rule           */
    const float* lse_dot;        /* fp32 [B, H, S] contiguous; given exactly when lse_out is      */
    float*       lse_out;        /* fp32 [B, H, S] contiguous; may be lse                         */
    float   softmax_scale;       /* the one given to la_fwd                                       */
    int32_t reserved0;           /* 0                                                              */
} la_attn_unshift_args;
int la_attn_unshift(const la_attn_unshift_args* args, void* stream);

/* la_attn_unshift_fp8 (added under ABI 9: a host detects it by symbol): la_attn_unshift with a row-scaled e4m3 result - the activation
 * of an fp8 output projection in one read of O and one 1-byte write. Everything la_attn_unshift does comes first, in its order and in
 * fp32, and nothing is rounded before the e4m3 conversion:
 *   y[h][:]          = float(o[b][s][h][:]) + shift[b][h / heads_per_vec][:]      one fp32 addition; shift NULL: nothing is added
 *   y[h][:]          = 0 when lse is given and lse[b][h][s] is +inf or -inf          the empty-row rule, per head; a NaN lse: the normal path
 *   lse_out[b][h][s] = fmaf(softmax_scale, lse_dot[b][h][s], lse[b][h][s])          only when lse_dot is given; an empty row keeps its lse
 * Heads share scales in groups of heads_per_scale (a divisor of num_heads), g = h / heads_per_scale.
 * DYNAMIC mode (descale_in NULL):
 *   amax             = max |y| over the heads_per_scale * head_dim elements of (b, s, g), as the unsigned maximum of the bit patterns:
 *                      order free, and any NaN wins
 *   row_descale[b][s][g] = max(amax, 2^-100) / 448       one IEEE division; fp32, by its own batch / row / group strides (elements)
 *   out              = e4m3fn_rne(clamp(y * (1 / row_descale[b][s][g]), -448, +448))     one IEEE division per (b, s, g); a NaN stays
 *   a NaN among the elements of a group makes that group's descale and its bytes NaN - no other group's, no other token's. No atomics;
 *   the order of the reduction is a function of the shape: two launches agree bit for bit. heads_per_scale == num_heads gives one
 *   scale per token, the row-wise scale of a scaled GEMM over H * D. amax is not read.
 * STATIC mode (descale_in given: fp32 [B] by descale_in_batch_stride, 0 = one element for every batch):
 *   out              = e4m3fn_rne(clamp(y * (1 / descale_in[b]), -448, +448)); row_descale is neither read nor written.
 *   amax             optional fp32 [B] by amax_batch_stride: amax[b] = max(amax[b], max |y| of the batch) as the unsigned maximum of the
 *                    bit patterns, la_qk_prep_fp8's semantics (zero it first for this call's maximum; any NaN wins; one integer
 *                    atomicMax per workgroup, no float atomics).
 * o bf16 / fp16 (B, S, H, D) and out e4m3 (B, S, H, D), each by its own strides (elements), last dimension contiguous; rows, heads and
 * batches of o start on 16-byte boundaries, those of out on 8-byte boundaries. There is NO in-place form. A scale group stays in the
 * registers of one wave between the reduction and the store: heads_per_scale * head_dim <= 16384 (LA_NORM_TOKEN's limit in la_qk_prep).
 * Errors (all before any HIP call), in this order: NULL args LA_ERR_NULL_ARG; struct_size LA_ERR_STRUCT_SIZE; NULL o or out, row_descale
 * and descale_in both NULL, exactly one of lse_dot / lse_out, or the two without lse, LA_ERR_NULL_ARG; o_dtype not bf16 / fp16
 * LA_ERR_DTYPE; a non-positive size, (with shift) heads_per_vec below 1 or not a divisor of num_heads, or heads_per_scale below 1 or
 * not a divisor of num_heads, LA_ERR_SHAPE; head_dim % 8 != 0 LA_ERR_HEAD_DIM; a negative stride of o, out or shift, o or shift off a
 * 16-byte boundary, out off an 8-byte one, a used stride of them that takes a row, head or batch start off one, LA_ERR_STRIDE; lse,
 * lse_dot, lse_out, row_descale, descale_in or amax off a 4-byte boundary, or a negative stride of the last three, LA_ERR_STRIDE;
 * out == o LA_ERR_UNSUPPORTED; heads_per_scale * head_dim above 16384, or more than 1024 heads (a workgroup keeps the empty-row flags
 * of every head of its 32 rows in LDS), LA_ERR_UNSUPPORTED; more than 2^31 - 1 tiles (B * ceil(S / 32), one workgroup each)
 * LA_ERR_SHAPE. NOT detected: any other overlap of out and o, a row_descale shorter than its strides say, a descale_in that is zero,
 * negative or not finite. */
typedef struct la_attn_unshift_fp8_args {
    uint32_t struct_size;        /* = sizeof(la_attn_unshift_fp8_args)                            */
    int32_t  o_dtype;            /* la_dtype of o: LA_DTYPE_BF16 or LA_DTYPE_FP16                 */
    int32_t  heads_per_vec;      /* query heads that share one shift row: H_q / H_kv              */
    int32_t  heads_per_scale;    /* heads that share one scale; divides num_heads                 */
    const void* o;               /* (B, S, H, D), last dimension contiguous                       */
    void*       out;             /* e4m3 (B, S, H, D) by its own strides; never o                 */
    int64_t o_batch_stride, o_row_stride, o_head_stride;          /* in elements                  */
    int64_t out_batch_stride, out_row_stride, out_head_stride;
    int32_t batch, seqlen, num_heads, head_dim;
    const float* shift;          /* fp32 [B, H / heads_per_vec, D] by the strides below; NULL = no shift */
    int64_t shift_batch_stride, shift_head_stride;
    const float* lse;            /* fp32 [B, H, S] contiguous; NULL = no empty-row rule           */
    const float* lse_dot;        /* fp32 [B, H, S] contiguous; given exactly when lse_out is      */
    float*       lse_out;        /* fp32 [B, H, S] contiguous; may be lse                         */
    float   softmax_scale;       /* the one given to la_fwd                                       */
    int32_t reserved0;           /* 0                                                              */
    float*  row_descale;         /* fp32 [B, S, H / heads_per_scale] by the strides below: written in the dynamic mode */
    int64_t row_descale_batch_stride, row_descale_row_stride, row_descale_group_stride;
    const float* descale_in;     /* fp32 [B] by the stride below (0: one element); given = the static mode */
    int64_t descale_in_batch_stride;
    float*  amax;                /* fp32 [B] by the stride below, accumulated, static mode only; NULL = not wanted */
    int64_t amax_batch_stride;
} la_attn_unshift_fp8_args;
int la_attn_unshift_fp8(const la_attn_unshift_fp8_args* args, void* stream);

/* fp8 V in one pass. la_fwd's e4m3 kernels do not read V (B, Sk, Hk, D): they stage pre-transposed, pre-swizzled V^T tiles
 * [B, Hk, ceil(Sk / 64)][head_dim (96: 128 rows, the last 32 zeros)][64 keys] from the front of the workspace, which la_fwd's prepare pass
 * writes from the e4m3 V unless LA_FLAG_V_PREPARED says they are there. la_v_prep_tiles writes the same bytes from V as its projection
 * wrote it:
 *   y  = float(x[b][s][h][d]) - shift[b][h][d]                       (shift NULL: y = float(x))
 *   z  = clamp(y * (1 / descale[b][h]), -448, +448)                  one IEEE division per (b, h); a NaN stays a NaN
 *   code = e4m3fn(z), round to nearest even
 * - for every element the byte la_qk_prep_smooth (LA_NORM_NONE, no rope, heads_per_scale 1, the same shift and descale) stores, in the
 * place la_fwd's prepare pass would put it; keys at and beyond seqlen are zeros. amax[b][h] = max(amax[b][h], max |y|) as the
 * unsigned maximum of the bit patterns, la_qk_prep_fp8's semantics (zero it first for this call's maximum; any NaN wins; one integer
 * atomicMax per workgroup, no float atomics: two launches write the same bytes). One read of x, one write of the tiles.
 * The call that follows: la_fwd with dtype LA_DTYPE_FP8_E4M3, flags | LA_FLAG_V_PREPARED, workspace = tiles and workspace_bytes >=
 * la_v_tiles_workspace_bytes(B, Hk, Sk, D), the descale given here as v_descale, and as v any 16-byte aligned buffer of B * Sk * Hk * D
 * bytes with valid strides (it is checked, never read: the tile buffer itself will do). That workspace size serves every
 * fixed-length, unsplit e4m3 la_fwd over these keys, with or without lists, with or without LA_FLAG_STATIC_SCHED: the tiles, then the
 * ticket counters. A dense launch whose keys la_fwd would cut into runs (la_fwd_workspace_bytes() above that size) has no prepared
 * form: la_fwd refuses it (LA_ERR_SEQLEN, or LA_ERR_WORKSPACE when the workspace is too small for the runs' partials).
 * Errors of la_v_prep_tiles (all before any HIP call), in this order: NULL args LA_ERR_NULL_ARG; struct_size LA_ERR_STRUCT_SIZE; NULL x
 * or tiles LA_ERR_NULL_ARG; in_dtype LA_ERR_DTYPE; a non-positive size LA_ERR_SHAPE; head_dim outside 64 / 96 / 128 / 192 / 256
 * LA_ERR_HEAD_DIM; reserved0 != 0 LA_ERR_UNSUPPORTED; a negative stride, x, shift or tiles off a 16-byte boundary, a used stride of x or
 * shift that takes a row, head or batch start off one, descale or amax off a 4-byte boundary, LA_ERR_STRIDE; more than 2^31 - 1 tiles
 * (B * Hk * ceil(S / 64)) LA_ERR_SHAPE. NOT detected: a tiles buffer shorter than la_v_tiles_bytes(), buffers that overlap.
 * la_v_tiles_bytes / la_v_tiles_workspace_bytes: B * Hk * ceil(Sk / 64) * 64 * (96: 128, else head_dim) bytes, and that plus the ticket
 * counters; a non-positive batch / num_heads_k or a negative seqlen_k LA_ERR_SHAPE, another head_dim LA_ERR_HEAD_DIM (as int64_t). */
typedef struct la_v_prep_tiles_args {
    uint32_t struct_size;        /* = sizeof(la_v_prep_tiles_args)                                */
    int32_t  in_dtype;           /* la_dtype of x: LA_DTYPE_BF16, LA_DTYPE_FP16 or LA_DTYPE_FP32  */
    const void* x;               /* (B, S, Hk, D), last dimension contiguous                      */
    int64_t x_batch_stride, x_row_stride, x_head_stride;          /* in elements                  */
    int32_t batch, seqlen, num_heads, head_dim;                   /* num_heads: kv heads          */
    const float* descale;        /* fp32 [B, Hk] by the strides below; NULL = 1.0                 */
    int64_t descale_batch_stride, descale_head_stride;
    const float* shift;          /* fp32 [B, Hk, D] by the strides below; NULL = no shift         */
    int64_t shift_batch_stride, shift_head_stride;
    float*  amax;                /* fp32 [B, Hk] by the strides below, accumulated; NULL = not wanted */
    int64_t amax_batch_stride, amax_head_stride;
    void*   tiles;               /* la_v_tiles_bytes() bytes, 16-byte aligned: the front of a la_fwd workspace */
    int32_t reserved0;           /* 0                                                              */
} la_v_prep_tiles_args;
int la_v_prep_tiles(const la_v_prep_tiles_args* args, void* stream);
int64_t la_v_tiles_bytes(int32_t batch, int32_t num_heads_k, int32_t seqlen_k, int32_t head_dim);
int64_t la_v_tiles_workspace_bytes(int32_t batch, int32_t num_heads_k, int32_t seqlen_k, int32_t head_dim);

/* How many workgroups of the kernel la_fwd runs for (head_dim, element size, flags) are resident at once on the current device:
 * compute units x workgroups per compute unit. A host that splits one attention into q-tile windows (la_fwd_args.q_tile_begin)
 * sizes them in whole rounds of this number. No counterpart in the reference (one launch per call). */
int la_device_slots(int head_dim, int element_size, uint32_t flags, int* compute_units, int* workgroups_per_cu);

/* What this binary was built from: "abi=9;src=<sha256[:16] of the kernel / API sources, generators and this header>;variant=0|1;
 * wrong_results=0|1;opts=<generator options and -D defines, empty for the product build>". The product build (variant=0) is generated
 * with NO generator option and NO define, whatever the environment of the build held; A/B and pricing builds (python -m
 * liteattention_amd.build --out=...) say variant=1, and wrong_results=1 when an option that changes the arithmetic went in. The Python
 * binding refuses a library in the default location whose record says variant / wrong_results or whose src differs from the tree
 * beside it. No counterpart in the reference (its build flags are only visible in setup.py's environment, hopper/setup.py:47-68). */
const char* la_build_info(void);

const char* la_status_string(int status);
int         la_abi_version(void);
int         la_last_hip_error(void);   /* hipError_t of the last failed launch on this thread */

#ifdef __cplusplus
}
#endif
#endif /* LITE_ATTENTION_AMD_H */
