// la_kernel_params.h — device-side parameter block (the slimmed-down Flash_fwd_params,
// /root/reference/hopper/_internal/cpp/flash.h:48-185) filled by la_api.hip from la_fwd_args.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace la {

struct FwdParams {
    const uint16_t* q;
    const uint16_t* k;
    const uint16_t* v;
    uint16_t* o;
    float* lse;
    int64_t q_batch_stride, q_row_stride, q_head_stride;   // elements
    int64_t k_batch_stride, k_row_stride, k_head_stride;
    int64_t v_batch_stride, v_row_stride, v_head_stride;
    int64_t o_batch_stride, o_row_stride, o_head_stride;
    int batch, seqlen_q, seqlen_k, num_heads;
    int h_ratio;            // num_heads / num_heads_k: query heads per K/V head (GQA/MQA; kv head = h / h_ratio)
    int q_tiles, k_tiles;
    int q_tile_begin;       // this launch covers q-tiles [q_tile_begin, q_tile_begin + q_tile_count) of every (batch, head):
    int q_tile_count;       // a window of the SAME problem (tensors, LSE and lists are indexed by the global q-tile)
    int list_q_tiles;       // rows of the skip lists per (batch, head). == q_tiles, except under LA_FLAG_HALF_VOTE (x64 kernel, head_dim 128): the
                            // lists are kept per 128-ROW HALF of a 256-row workgroup item: list_q_tiles = ceil(seqlen_q / 128), and item m
                            // reads / writes rows 2 m and 2 m + 1 (q_tiles, q_tile_begin, q_tile_count stay in items of 256 rows)
    int half_vote;          // 1 = that mode
    int seq_cap;            // int32 slots reserved in LDS for the expanded tile sequence
    int walk_buffers;       // x64 kernels: 2 = a second walk buffer (tile sequence + vote / range-end flags) fits in LDS beside the first: the next
                            // item's read list is expanded while this item's write list is serialised; 1 = serial (very long key sequences, head_dim > 128)
    float scale_log2;       // softmax_scale * log2(e)   (flash_api.cpp:125-126)
    float rescale_tau;      // x64 kernel: O/l follow the running max only when it grew by more than this (log2 units)
    float thr;
    unsigned* work_counter; // x64 + lists: zeroed ticket counter in caller workspace -> persistent workgroups take work items
                            // dynamically (skip lists make items unequal); nullptr -> one workgroup per item, static XCD map
    const void* read_list;  // rows of int32_t, or of int16_t when list_int16 (LA_FLAG_LIST_INT16): same geometry, offsets in ELEMENTS
    void* write_list;
    const int* must_do_list;   // int32 in both forms
    int must_do_is_1d;
    // fp8 only: per-(batch, head) descales, NULL = 1.0 (flash_api.cpp:1003-1022); strides in elements
    const float* q_descale;
    const float* k_descale;
    const float* v_descale;
    int64_t q_descale_batch_stride, q_descale_head_stride;
    int64_t k_descale_batch_stride, k_descale_head_stride;
    int64_t v_descale_batch_stride, v_descale_head_stride;
    // variable-length batches (dense only): device prefix sums int32[batch + 1]; seqlen_q / seqlen_k / q_tiles / k_tiles above are
    // then the MAXIMA over the batch, lse is (H, total_q). nullptr = fixed length.
    const int* cu_seqlens_q;
    const int* cu_seqlens_k;
    // la_fwd_head_thr: the vote threshold of the item of (batch or packed sequence b, QUERY head h) is thr_head[b * thr_bs + h * thr_hs] and thr
    // above is not read; nullptr (la_fwd, and every dense launch) = thr for all. Device fp32, strides in elements.
    const float* thr_head;
    int64_t thr_bs, thr_hs;
    int64_t total_q;
    int list_int16;         // 1 = read_list / write_list hold int16_t (wave-uniform: the shells pick the element type of the list readers / writers by it)
};
// The threshold the item of (b, h) votes with: one wave-uniform load per item, taken before the item's parameter block is filled.
__device__ __forceinline__ float item_thr(const FwdParams& p, int b, int h) {
    return p.thr_head != nullptr ? p.thr_head[b * p.thr_bs + h * p.thr_hs] : p.thr;
}

// Varlen launches (la_fwd_args.cu_seqlens_*): sequence b's own rows and lengths.
struct SeqView {
    int seqlen_q, seqlen_k, k_tiles;
    int64_t q_off, k_off, v_off, o_off;   // element offsets of the sequence's first row in q / k / v / o
    float* lse_row0;                      // &lse[row 0 of this (batch, head)] (may be derived from nullptr: check p.lse)
};
__device__ __forceinline__ SeqView seq_view(const FwdParams& p, int b, int h, int block_n) {
    SeqView s;
    const int q0 = p.cu_seqlens_q[b], k0 = p.cu_seqlens_k[b];
    s.seqlen_q = min(max(p.cu_seqlens_q[b + 1] - q0, 0), p.seqlen_q);
    s.seqlen_k = min(max(p.cu_seqlens_k[b + 1] - k0, 0), p.seqlen_k);
    s.k_tiles = (s.seqlen_k + block_n - 1) / block_n;
    s.q_off = q0 * p.q_row_stride; s.k_off = k0 * p.k_row_stride; s.v_off = k0 * p.v_row_stride; s.o_off = q0 * p.o_row_stride;
    s.lse_row0 = p.lse + static_cast<int64_t>(h) * p.total_q + q0;
    return s;
}

// Dynamic work distribution: zero the ticket counter on `stream` and return the persistent grid (workgroups per CU x CUs,
// capped by the number of items). work_counter == nullptr -> static: one workgroup per item.
int compute_units();
inline hipError_t prepare_work_queue(FwdParams& p, bool skipable, int total, int wg_per_cu, hipStream_t stream, int* grid) {
    *grid = total;
    if (!skipable) p.work_counter = nullptr;        // dense: every item costs the same, the static map is balanced
    if (p.work_counter == nullptr) return hipSuccess;
    constexpr size_t kWorkQueueBytes = 16 * 64;     // == kSchedWorkspaceBytes of la_api.hip (what la_fwd_workspace_bytes asks the caller for)
    static_assert(kWorkQueueBytes == 1024, "la_api.hip promises callers a 1024-byte scheduler workspace: change both together");
    const hipError_t err = hipMemsetAsync(p.work_counter, 0, kWorkQueueBytes, stream);       // 8 ticket queues, one 64-byte line each (+ 8 lines the LA_SCHED_GANG A/B build counts finished items in)
    if (err != hipSuccess) return err;
    const int slots = wg_per_cu * compute_units();
    *grid = total < slots ? total : slots;
    return hipSuccess;
}

size_t fwd_lds_bytes_v2(int head_dim, int k_tiles, int* seq_cap_out);
hipError_t launch_fwd_bf16_v2(const FwdParams& p, int head_dim, bool skipable, bool f16, hipStream_t stream);   // 128-row hipcc-scheduled template: head_dim 64; 128 / 256 as the A/B kernels (LA_FLAG_KERNEL_128ROW)
int x64_workgroups_per_cu(int head_dim);      // resident workgroups per CU of the hand-scheduled kernels: 1
hipError_t launch_fwd_x64(const FwdParams& p, int head_dim, bool skipable, bool f16, hipStream_t stream);  // p.half_vote: the half-vote form (head_dim 128, lists only)  // 1 wave/SIMD; head_dim 128: 64 rows/wave, q-tile 256; 256: 32 rows/wave, q-tile 128
hipError_t launch_fwd_x64_fp8(const FwdParams& p, bool skipable, int p_mode, int head_dim, hipStream_t stream);   // 1 wave/SIMD, 64 rows/wave; p.v = V^T workspace
size_t fp8_workspace_bytes(int batch, int num_heads_k, int k_tiles, int head_dim);   // prepared V^T tiles: 64 keys x head_dim bytes each
hipError_t launch_prep_v_fp8(const void* v, int64_t v_batch_stride, int64_t v_row_stride, int64_t v_head_stride,
                             void* vt, int batch, int seqlen_k, int num_heads_k, int k_tiles, int head_dim, hipStream_t stream,
                             const int* cu_seqlens_k = nullptr);
// la_v_prep_tiles (la_prep_fp8.hip): the quantizing front end of the same tile writer - x as the projection wrote it -> the V^T tiles.
// Checked and filled by la_api.hip. Strides in elements.
struct VPrepTilesParams {
    const void* x;               // (B, S, Hk, D) bf16 / fp16 / fp32 by x_bs / x_rs / x_hs
    uint8_t* tiles;              // [B, Hk, Kt][D (96: 128)][64]: fp8_workspace_bytes(B, Hk, Kt, D) bytes
    const float* descale;        // [B, Hk] by ds_bs / ds_hs; NULL = 1.0
    const float* shift;          // [B, Hk, D] by sh_bs / sh_hs; NULL = none
    float* amax;                 // [B, Hk] by am_bs / am_hs: running maximum of |x - shift| as its bit pattern; NULL = not wanted
    int64_t x_bs, x_rs, x_hs, ds_bs, ds_hs, sh_bs, sh_hs, am_bs, am_hs;
    int batch, seqlen, num_heads, head_dim, k_tiles;
};
hipError_t launch_v_prep_tiles(const VPrepTilesParams& p, int in_dtype, hipStream_t stream);      // in_dtype: 0 bf16, 1 fp16, 3 fp32
hipError_t launch_empty_k_fill(uint16_t* o, float* lse, int64_t o_batch_stride, int64_t o_row_stride, int64_t o_head_stride,
                               int batch, int seqlen_q, int num_heads, int head_dim_v, hipStream_t stream);
hipError_t launch_skip_list_stats(const void* list, int list_elem_size, int rows, int k_tiles, int64_t* out, hipStream_t stream);
hipError_t launch_skip_list_stats_heads(const void* list, int list_elem_size, int heads, int q_tiles, int k_tiles, int64_t* out, hipStream_t stream);   // out[heads]: heads = batch * num_heads
hipError_t launch_blockmask_to_lists(const uint8_t* mask, int64_t mask_batch_stride, int64_t mask_head_stride, int batch,
                                     int num_heads, int q_tiles, int k_tiles, const int32_t* q_tiles_valid,
                                     const int32_t* k_tiles_valid, void* lists, int list_elem_size, int32_t* empty_rows, hipStream_t stream);
hipError_t launch_combine(const void* o_partial, bool partial_is_16bit, bool f16, const float* lse_partial, uint16_t* o,
                          float* lse, int num_splits, int batch, int seqlen_q, int num_heads, int head_dim_v,
                          hipStream_t stream, bool out_f32 = false, int64_t o_batch_stride = 0, int64_t o_row_stride = 0,
                          int64_t o_head_stride = 0);      // strides (elements) of a strided 16-bit result; 0 = contiguous

hipError_t launch_combine_list(const void* const* o_partials, bool partial_is_16bit, bool f16, const float* const* lse_partials, uint16_t* o,
                               float* lse, int num_splits, int batch, int seqlen_q, int num_heads, int head_dim_v, hipStream_t stream,
                               bool out_f32 = false);
hipError_t launch_output_error(const void* out, int out_dtype, int64_t o_bs, int64_t o_rs, int64_t o_hs, const void* ref, int ref_dtype,
                               int64_t r_bs, int64_t r_rs, int64_t r_hs, int batch, int seqlen, int num_heads, int head_dim, int rows_per_bin,
                               double* stats, hipStream_t stream);   // la_output_error: fp64 [batch, heads, bins, 6], every element written

// la_qk_prep (la_prep_qk.hip): what the kernels read, checked and filled by la_api.hip. Strides in elements.
struct QkPrepParams {
    const void* x;
    void* out;
    const float* weight;         // NULL = ones
    const float* table[3];       // fp32 [extent_a, pairs_a, 2] (cos, sin); only read when rotate != 0 and pairs_a > 0
    int64_t x_bs, x_rs, x_hs, o_bs, o_rs, o_hs;
    int64_t tokens;              // batch * seqlen
    int seqlen, num_heads, head_dim;
    int norm_mode;               // 0 none, 1 token, 2 head (la_norm_mode)
    int rotate;                  // 0: no table is read
    int ext1, ext2;              // extents of axes 1 and 2: position p -> (p / (ext1 * ext2), (p / ext2) % ext1, p % ext2)
    int pairs[3];
    int pos_offset;
    float eps;
    // la_qk_prep_fp8 only (la_qk_prep leaves them zero): the e4m3 output form. Scale group of head h = h / heads_per_scale.
    const float* descale;        // [batch, groups] by the strides below; NULL = 1.0. out = e4m3(clamp(y * (1 / descale), +-448))
    float* amax;                 // [batch, groups] running maximum of |y| (as the unsigned maximum of its bit pattern); NULL = not wanted
    int64_t ds_bs, ds_hs, am_bs, am_hs;
    int heads_per_scale;         // >= 1, divides num_heads; num_heads <= kQkPrepScaleSlots
    // la_qk_prep_smooth only (the others leave them zero): every pointer NULL = that step off
    const float* shift;          // [batch, heads, head_dim] by sh_bs / sh_hs: out and amax are taken from y - shift
    float* colsum_part;          // [4 part_blocks, batch, heads, head_dim] contiguous: sums of the unshifted y over the rows of each part
    const float* dot_vec;        // [batch, heads / heads_per_dot, head_dim] by dv_bs / dv_hs
    float* dot_out;              // [batch, heads, seqlen] contiguous: sum_d y * dot_vec, of the unshifted y
    int64_t sh_bs, sh_hs, dv_bs, dv_hs;
    int heads_per_dot;
    int batch;
    int part_rows, part_blocks;  // rows of a part; part p = rows [p part_rows, (p + 1) part_rows) of a batch; 4 parts per block
    // the _rows entry points only (the others leave the pointers NULL): out row s of batch b is made from row src_rows[b map_bs + s] of x
    // (NULL: s) and rotated as position pos_offset + positions[b map_bs + s] (NULL: the source row). Entries are clamped, never trusted.
    const int32_t* src_rows;     // [batch or 1][seqlen]
    const int32_t* positions;    // [batch or 1][seqlen]
    int64_t map_bs;              // elements between the tables of two batches; 0: one table for every batch
    int src_seqlen;              // rows of x: a source row is clamped into [0, src_seqlen)
    int pos_limit;               // e0 * e1 * e2 (1 when nothing rotates): a position is clamped into [0, pos_limit)
};
constexpr int kQkPrepScaleSlots = 1024;      // heads whose scale and running amax a workgroup keeps in LDS (la_qk_prep_fp8)
constexpr int kQkPrepSumSlots = 16;          // chunks of 8 columns a thread keeps running column sums for in LDS (la_qk_prep_smooth): 128 KiB
// dtypes: 0 bf16, 1 fp16, 3 fp32 (in only), 2 e4m3 (out only). mode: 0 la_qk_prep (16-bit out); la_qk_prep_fp8: 1 quantize, 2 the amax pass
// alone (p.out == NULL); la_qk_prep_smooth with a shift, column sums or row dots: 3 with out, 4 without
hipError_t launch_qk_prep(const QkPrepParams& p, int in_dtype, int out_dtype, int mode, hipStream_t stream);
// la_qk_prep_smooth: rows of a part and blocks of 4 parts for a sequence length - the one place the row -> part map is decided
inline int qk_prep_part_rows(int seqlen) { const int r = static_cast<int>((static_cast<int64_t>(seqlen) + 1023) / 1024); return r < 16 ? 16 : r; }
inline int qk_prep_part_blocks(int seqlen) {
    const int r = qk_prep_part_rows(seqlen);
    return static_cast<int>(((static_cast<int64_t>(seqlen) + r - 1) / r + 3) / 4);
}
int qk_prep_sum_slots(const QkPrepParams& p);      // chunks per thread the column sums of this shape need (<= kQkPrepSumSlots or unsupported)
hipError_t launch_colsum_finish(const float* part, int n_parts, int batch, int num_heads, int head_dim, int seqlen, float* mean,
                                int64_t m_bs, int64_t m_hs, hipStream_t stream);

// la_v_colstats / la_attn_unshift (la_prep_v.hip): checked and filled by la_api.hip. Strides in elements.
struct VColstatsParams {
    const void* x;               // (B, S, H, D) by x_bs / x_rs / x_hs
    float* stat_part;            // [n_parts, 3, B, H, D] contiguous: sum, minimum, maximum over the rows of each part
    int64_t x_bs, x_rs, x_hs;
    int batch, seqlen, num_heads, head_dim;
    int n_parts, part_rows;
};
// Rows of a part: about kVColstatsThreads threads of 8 columns each (two waves per SIMD on 256 compute units), never fewer than 16
// rows per part. The one place the row -> part map of la_v_colstats is decided: a function of (S, H, D) alone.
constexpr int64_t kVColstatsThreads = 131072;
inline int v_colstats_part_rows(int seqlen, int num_heads, int head_dim) {
    const int64_t chunks = static_cast<int64_t>(num_heads) * ((head_dim + 7) / 8);
    const int64_t r = (static_cast<int64_t>(seqlen) * chunks + kVColstatsThreads - 1) / kVColstatsThreads;
    return r < 16 ? 16 : (r > 0x7fffffffLL ? 0x7fffffff : static_cast<int>(r));
}
inline int v_colstats_parts(int seqlen, int num_heads, int head_dim) {
    const int64_t r = v_colstats_part_rows(seqlen, num_heads, head_dim);
    return static_cast<int>((static_cast<int64_t>(seqlen) + r - 1) / r);
}
hipError_t launch_v_colstats(const VColstatsParams& p, int in_dtype, hipStream_t stream);      // in_dtype: 0 bf16, 1 fp16, 3 fp32
hipError_t launch_v_colstats_finish(const float* part, int n_parts, int batch, int num_heads, int head_dim, int seqlen, float* mean,
                                    int64_t m_bs, int64_t m_hs, float* amax, int64_t a_bs, int64_t a_hs, hipStream_t stream);
struct AttnUnshiftParams {
    const void* o;               // bf16 / fp16 (B, S, H, D) by o_bs / o_rs / o_hs
    void* out;                   // bf16 / fp16 / fp32 by out_bs / out_rs / out_hs; may be o
    const float* shift;          // [B, H / heads_per_vec, D] by sh_bs / sh_hs; NULL = nothing added
    const float* lse;            // [B, H, S] contiguous; NULL = no empty-row rule
    const float* lse_dot;        // [B, H, S]; given exactly when lse_out is
    float* lse_out;              // [B, H, S]; may be lse
    int64_t o_bs, o_rs, o_hs, out_bs, out_rs, out_hs, sh_bs, sh_hs;
    int batch, seqlen, num_heads, head_dim, heads_per_vec;
    float softmax_scale;
    // la_attn_unshift_fp8 only (la_attn_unshift leaves them zero): out is e4m3. Scale group of head h = h / heads_per_scale.
    float* row_descale;          // [B, S, H / heads_per_scale] by rd_bs / rd_rs / rd_gs: written in the dynamic mode (descale_in NULL)
    const float* descale_in;     // [B] by di_bs (0: one element for every batch); given = the static mode, row_descale is not written
    float* amax;                 // [B] by am_bs, static mode: running maximum of |y| as the unsigned maximum of its bit pattern; NULL = not wanted
    int64_t rd_bs, rd_rs, rd_gs, di_bs, am_bs;
    int heads_per_scale;         // >= 1, divides num_heads; heads_per_scale * head_dim <= kAttnOutFp8MaxGroup
};
constexpr int kAttnOutFp8MaxGroup = 16384;   // elements of a scale group (la_attn_unshift_fp8): a wave keeps them in registers, 32 chunks of 8 a lane
constexpr int kAttnOutFp8MaxHeads = 1024;    // heads whose empty-row flags of 32 rows a workgroup keeps in LDS
constexpr int kAttnOutFp8Rows = 32;          // rows of a workgroup's tile: one 128-byte line of lse per head
// out_dtype: 0 bf16, 1 fp16, 3 fp32 (la_attn_unshift), 2 e4m3 (la_attn_unshift_fp8: one workgroup per tile of kAttnOutFp8Rows rows of a batch)
hipError_t launch_attn_unshift(const AttnUnshiftParams& p, int o_dtype, int out_dtype, hipStream_t stream);

}  // namespace la
