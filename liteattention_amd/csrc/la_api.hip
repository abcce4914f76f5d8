// la_api.hip — the C-ABI (include/lite_attention_amd.h): validation, parameter fill, dispatch.
//
// Replaces mha_fwd + set_params_fprop + run_mha_fwd of the reference
// (/root/reference/hopper/_internal/cpp/flash_api.cpp:45-163, 362-380, 667-1249). The checks mirror
// the reference's TORCH_CHECKs (cited per check) but return codes instead of throwing; the Python
// layer turns codes into the reference's exception types.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lite_attention_amd.h"
#include "la_fwd_shell.h"      // fwd_lds_size_x64, X_LDS_LIMIT: the LDS a launch of the hand-scheduled kernels needs
#include "la_kernel_params.h"
#include "la_tiles.h"

namespace {
thread_local int g_last_hip_error = 0;     // per-thread error detail of the last failed launch; the only state in the library

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the tail of every entry point that launches: the HIP error, if any, goes to la_last_hip_error()
int launch_status(hipError_t err) {
    if (err == hipSuccess) return LA_OK;
    g_last_hip_error = static_cast<int>(err);
    return LA_ERR_LAUNCH;
}

// Every row, head and batch start of a (batch, seqlen, heads, D) tensor on a boundary of `align` bytes: the pointer, and every stride
// that is used, a multiple of `unit` elements (a row of 8 elements is 16 bytes of bf16 / fp16, two 16-byte halves of fp32, 8 bytes of
// e4m3). No stride is negative.
bool rows_aligned(const void* ptr, unsigned align, int64_t unit, int64_t bs, int64_t rs, int64_t hs, int batch, int seqlen, int heads) {
    return bs >= 0 && rs >= 0 && hs >= 0 && (reinterpret_cast<uintptr_t>(ptr) & (align - 1)) == 0 && (seqlen <= 1 || rs % unit == 0) &&
           (heads <= 1 || hs % unit == 0) && (batch <= 1 || bs % unit == 0);
}
// ... with unit and alignment from the la_dtype: 16-byte rows, 8-byte rows of e4m3
bool rows_aligned(const void* ptr, int32_t dtype, int64_t bs, int64_t rs, int64_t hs, int batch, int seqlen, int heads) {
    return rows_aligned(ptr, dtype == LA_DTYPE_FP8_E4M3 ? 8u : 16u, dtype == LA_DTYPE_FP32 ? 4 : 8, bs, rs, hs, batch, seqlen, heads);
}

bool is_input_dtype(int32_t d) { return d == LA_DTYPE_BF16 || d == LA_DTYPE_FP16 || d == LA_DTYPE_FP32; }   // what the passes around la_fwd read (and la_combine writes)

// Kernel selection is a pure function of the arguments (no environment variables, no process-wide statics):
//   bf16 / fp16 head_dim 128: the 256-row hand-scheduled kernel (x64) unless LA_FLAG_KERNEL_128ROW asks for the 128-row one (v2);
//   head_dim 256: the hand-scheduled kernel in its 32-rows-per-wave form (q-tile 128) unless LA_FLAG_KERNEL_128ROW asks for the
//   hipcc-scheduled v2 instantiation (same tiles); head_dim 96 / 192: the 128 / 256 hand-scheduled forms with three quarters of
//   the fragments (no v2 instantiation: LA_ERR_HEAD_DIM under LA_FLAG_KERNEL_128ROW, hosts pad to 128 / 256 then);
//   head_dim 64: the hand-scheduled kernel with 8 + 8 fragments per tile (q-tile 256) unless LA_FLAG_KERNEL_128ROW asks for v2 (q-tile 128);
//   fp8 head_dim 128: x64-fp8. The skip lists are indexed by the selected kernel's tile, so
//   la_get_tile_sizes_ex and la_fwd must agree on it: both call uses_128row().
constexpr uint32_t kKnownFlags = LA_FLAG_V_PREPARED | LA_FLAG_STATIC_SCHED | LA_FLAG_KERNEL_128ROW | LA_FLAG_EXACT_RESCALE |
                                LA_FLAG_FP8_MFMA_ROWSUM | LA_FLAG_FP8_ENCODED_P | LA_FLAG_HALF_VOTE | LA_FLAG_LIST_INT16;
constexpr int kListInt16MaxRow = 32767;           // LA_FLAG_LIST_INT16: a row of k_tiles + 1 entries whose values (tile indices, counts <= k_tiles) fit int16
bool uses_128row(int head_dim, int element_size, uint32_t flags) {      // the flag changes the q-tile (256 -> 128 rows) at head dims 64 and 128
    return element_size == 2 && (head_dim == 128 || head_dim == 64) && (flags & LA_FLAG_KERNEL_128ROW) != 0;
}
// LA_FLAG_HALF_VOTE: the hand-scheduled kernel with skip lists per 128-row half of its 256-row workgroup (bf16 / fp16 head dims 64 / 96 / 128,
// the kernels with a 256-row q-tile; no effect elsewhere, and LA_FLAG_KERNEL_128ROW - another kernel with the same list geometry - wins
// when both are set)
bool uses_half_vote(int head_dim, int element_size, uint32_t flags) {
    return element_size == 2 && (head_dim == 128 || head_dim == 96 || head_dim == 64) && (flags & LA_FLAG_HALF_VOTE) != 0 &&
           (flags & LA_FLAG_KERNEL_128ROW) == 0;
}
// Long DENSE key ranges (hand-scheduled kernels; e4m3 too: la_fwd's fp8 branch). A workgroup keeps the tile-address table of its walk in LDS, which bounds the key
// tiles of ONE launch (~4 800 at head_dim <= 128, ~1 600 at 192 / 256). A skip list names its tiles over the whole key range and keeps that
// bound (LA_ERR_SEQLEN); a dense launch does not need it: with the workspace la_fwd_workspace_bytes() asks for, la_fwd cuts the keys into
// the fewest equal runs of tiles that fit, runs them as launches on partial O / LSE buffers in the workspace and merges them by LSE
// (la_combine's kernel) - the reference has no such bound (its producer reads the list from global memory, mainloop...:47-115).
int dense_tiles_per_launch(int head_dim, int element_size) {
    int lo = 1, hi = 1 << 20;                         // largest k_tiles whose walk fits (the LDS bytes grow with k_tiles)
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (la::fwd_lds_size_x64(element_size, head_dim, mid).bytes <= la::X_LDS_LIMIT) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// What la_skip_list_stats_ex, la_skip_list_stats_heads and la_blockmask_to_lists_ex check of a list's geometry [n_batch, num_heads, q_tiles,
// k_tiles + 1] of list_elem_size-byte entries, in their order (strides_ok: the one check the mask entry point has between them).
int list_geometry_status(int32_t list_elem_size, int32_t n_batch, int32_t num_heads, int32_t q_tiles, int32_t k_tiles, bool strides_ok = true) {
    if (list_elem_size != 2 && list_elem_size != 4) return LA_ERR_DTYPE;
    if (n_batch <= 0 || num_heads <= 0 || q_tiles <= 0 || k_tiles <= 0) return LA_ERR_SHAPE;
    if (list_elem_size == 2 && k_tiles + 1 > kListInt16MaxRow) return LA_ERR_SEQLEN;
    if (!strides_ok) return LA_ERR_STRIDE;
    if (static_cast<int64_t>(n_batch) * num_heads * q_tiles > 0x7fffffffLL) return LA_ERR_SHAPE;    // one wave or workgroup per row
    return LA_OK;
}
// What la_combine and la_combine_list check alike, behind their NULL checks
int combine_status(const void* o, int32_t o_dtype, int32_t partial_is_16bit, int32_t num_splits, int32_t max_splits, int32_t batch,
                   int32_t seqlen_q, int32_t num_heads, int32_t head_dim_v) {
    if (!is_input_dtype(o_dtype)) return LA_ERR_DTYPE;
    if (o_dtype == LA_DTYPE_FP32 && partial_is_16bit) return LA_ERR_DTYPE;      // an fp32 result is the merge of fp32 partials
    if (num_splits <= 0 || num_splits > max_splits || batch <= 0 || seqlen_q <= 0 || num_heads <= 0 || head_dim_v <= 0) return LA_ERR_SHAPE;
    if (head_dim_v % 8 != 0) return LA_ERR_HEAD_DIM;
    if (!aligned16(o)) return LA_ERR_STRIDE;
    return LA_OK;
}
constexpr uint64_t kSchedWorkspaceBytes = 1024;   // 16 ticket / steal counters of 64 bytes, all of them zeroed by prepare_work_queue (no slack)

// The caller's workspace of ONE la_fwd call, in the order it lies there: the prepared V^T tiles (e4m3 only; split: those of ONE run - the
// runs follow each other on the stream), the ticket block, then - split only - the partial O and the partial LSE of the n runs. The one
// description of it: la_fwd_workspace_bytes returns `total`, la_fwd checks workspace_bytes against it and takes every pointer from it.
struct FwdWorkspace {
    bool split;                                   // a dense key range longer than one launch's walk, cut into n equal runs of chunk_tiles
    int n, chunk_tiles;                           // (not split: 1 run of all the key tiles)
    uint64_t tickets, o_part, lse_part, total;    // byte offsets (the tiles are at 0) and the bytes in all
    uint64_t o_bytes, lse_bytes;                  // one run's partial O (16-bit for every input type: bf16 / fp16 as the inputs, bf16 for e4m3) and LSE
};
// k_tiles: of the whole key range. may_split = false: one launch whatever the length. A launch that fits never reaches the bisection.
FwdWorkspace fwd_workspace(const la_fwd_args* a, int esize, int k_tiles, bool may_split) {
    const bool fp8 = esize == 1, skipable = a->read_list != nullptr, x64 = fp8 || !(a->flags & LA_FLAG_KERNEL_128ROW);
    FwdWorkspace w;
    w.split = may_split && x64 && !skipable && a->cu_seqlens_q == nullptr && la::fwd_lds_size_x64(esize, a->head_dim, k_tiles).bytes > la::X_LDS_LIMIT;
    w.n = 1; w.chunk_tiles = k_tiles; w.o_bytes = w.lse_bytes = 0;
    if (w.split) {
        const int per = dense_tiles_per_launch(a->head_dim, esize);
        w.n = (k_tiles + per - 1) / per;
        w.chunk_tiles = (k_tiles + w.n - 1) / w.n;
        w.o_bytes = ((static_cast<uint64_t>(a->batch) * a->seqlen_q * a->num_heads * a->head_dim_v * 2) + 15) & ~15ull;
        w.lse_bytes = static_cast<uint64_t>(a->batch) * a->num_heads * a->seqlen_q * 4;   // (exact: the merge reads run s at s * one partial; the O partials come first, so each is 16-byte aligned)
    }
    // ticket counters: e4m3 and split launches always have room for them; else launches with lists and dense launches of the hand-scheduled
    // kernels (the 128-row template keeps the static map for dense), unless LA_FLAG_STATIC_SCHED
    const bool tickets = fp8 || w.split || ((skipable || x64) && !(a->flags & LA_FLAG_STATIC_SCHED));
    w.tickets = fp8 ? la::fp8_workspace_bytes(a->batch, a->num_heads_k, w.chunk_tiles, a->head_dim) : 0;
    w.o_part = w.tickets + (tickets ? kSchedWorkspaceBytes : 0);
    w.lse_part = w.o_part + w.n * w.o_bytes;
    w.total = w.lse_part + w.n * w.lse_bytes;
    return w;
}
constexpr float kRescaleTauBf16 = 8.0f;           // lazy-rescale slack of the x64 kernel, log2 units (HISTORY.md section 3.1)

// ---- la_fwd / la_fwd_head_thr: check, then fill, then dispatch. What the checks compute on their way and the later steps need:
struct FwdChecked {
    bool fp8, f16, varlen, half_vote, ws_ok;       // f16: same kernels as bf16 with the fp16 MFMA and conversions; ws_ok: the workspace holds `ws`
    int esize, bm, bn, k_tiles;
    int q_tiles, list_q_tiles, q_tile_begin, q_tile_count;      // the window in the KERNEL's items (half-vote: pairs of list rows)
    FwdWorkspace ws;
};
// Every check of la_fwd, in the order that decides the first error code. With no keys (seqlen_k == 0) nothing is walked: the checks stop
// behind the varlen ones and c holds nothing from `ws_ok` on.
int fwd_check(const la_fwd_args* a, FwdChecked& c) {
    if (a == nullptr) return LA_ERR_NULL_ARG;
    if (a->struct_size != sizeof(la_fwd_args)) return LA_ERR_STRUCT_SIZE;
    if (a->dtype != LA_DTYPE_BF16 && a->dtype != LA_DTYPE_FP16 && a->dtype != LA_DTYPE_FP8_E4M3) return LA_ERR_DTYPE;   // flash_api.cpp:715
    const bool fp8 = c.fp8 = a->dtype == LA_DTYPE_FP8_E4M3;
    c.f16 = a->dtype == LA_DTYPE_FP16;
    const int esize = c.esize = fp8 ? 1 : 2;
    if (!a->q || !a->o || ((!a->k || !a->v) && a->seqlen_k != 0)) return LA_ERR_NULL_ARG;   // empty K/V tensors may be NULL
    if (a->batch <= 0 || a->seqlen_q <= 0 || a->seqlen_k < 0 || a->num_heads <= 0 || a->num_heads_k <= 0 ||
        a->head_dim <= 0 || a->head_dim_v <= 0)
        return LA_ERR_SHAPE;                                                             // flash_api.cpp:776-778
    if (a->num_heads % a->num_heads_k != 0) return LA_ERR_SHAPE;                          // flash_api.cpp:777
    if (a->head_dim % (fp8 ? 16 : 8) != 0) return LA_ERR_HEAD_DIM;                         // flash_api.cpp:854-856
    if (a->head_dim_v != a->head_dim) return LA_ERR_UNSUPPORTED;
    if (a->reserved0 != 0 || (a->flags & ~kKnownFlags) != 0) return LA_ERR_UNSUPPORTED;
    const bool skipable = a->read_list != nullptr;                                       // is_skipable, flash_api.cpp:931
    if ((a->flags & LA_FLAG_LIST_INT16) && !skipable && a->write_list == nullptr)
        return LA_ERR_UNSUPPORTED;                     // the flag types the list pointers: a launch without lists has nothing it could mean
    const int trc = la_get_tile_sizes_ex(a->head_dim, esize, a->flags, &c.bm, &c.bn);
    if (trc != LA_OK) return trc;
    if (a->block_m != c.bm || a->block_n != c.bn) return LA_ERR_TILE_MISMATCH;
    if (skipable != (a->write_list != nullptr)) return LA_ERR_LISTS;
    // 16-byte vector access on every row: row/head/batch strides multiples of 8 elements, base aligned
    const int64_t strides[] = {a->q_batch_stride, a->q_row_stride, a->q_head_stride, a->k_batch_stride,
                               a->k_row_stride,   a->k_head_stride, a->v_batch_stride, a->v_row_stride,
                               a->v_head_stride,  a->o_batch_stride, a->o_row_stride,  a->o_head_stride};
    for (int i = 0; i < 12; ++i) {                                                       // flash_api.cpp:726-728 (+alignment)
        const int64_t s = strides[i];
        const int gran = (fp8 && i < 9) ? 16 : 8;                                        // 16-byte rows: 16 fp8 / 8 bf16 elements
        if (s % gran != 0 || s < 0) return LA_ERR_STRIDE;
    }
    if (a->o_row_stride > 0x3fffffff || a->q_row_stride > 0x3fffffff)
        return LA_ERR_STRIDE;                                                             // byte strides kept in 32 bits (the row offset itself is 64-bit)
    // K / V: a lane's DMA offset inside a key tile, row_in_tile * row_stride_bytes + chunk + bias, is an UNSIGNED 32-bit register of the
    // load (hand-scheduled bodies: rows 0 .. 63, chunk < 512, bias <= 3072) or an int (128-row template: rows 0 .. 14 and 0 .. 7 of a wave's
    // slice): 63 * 2^26 + 3584 < 2^32 and 14 * 2^26 < 2^31. LA_MAX_KV_ROW_STRIDE_BYTES is the largest power of two inside both.
    if (a->k_row_stride > LA_MAX_KV_ROW_STRIDE_BYTES / esize || a->v_row_stride > LA_MAX_KV_ROW_STRIDE_BYTES / esize)
        return LA_ERR_STRIDE;
    if (!aligned16(a->q) || !aligned16(a->k) || !aligned16(a->v) || !aligned16(a->o)) return LA_ERR_STRIDE;

    const bool varlen = c.varlen = a->cu_seqlens_q != nullptr || a->cu_seqlens_k != nullptr;
    if (varlen) {                                                                        // flash_api.cpp:736-760
        if (a->cu_seqlens_q == nullptr || a->cu_seqlens_k == nullptr) return LA_ERR_NULL_ARG;
        if (skipable && ((a->flags & LA_FLAG_KERNEL_128ROW) || (a->head_dim > 128 && !fp8)))
            return LA_ERR_UNSUPPORTED;                                                    // lists + cu_seqlens: the hand-scheduled kernels, head_dim <= 128 (e4m3: every head dim)
        if (a->total_q < 0 || a->q_tile_count != 0) return LA_ERR_SHAPE;
    }
    if (a->seqlen_k == 0) return LA_OK;

    c.k_tiles = (a->seqlen_k + c.bn - 1) / c.bn;
    c.ws = fwd_workspace(a, esize, c.k_tiles, true);
    c.ws_ok = a->workspace != nullptr && aligned16(a->workspace) && a->workspace_bytes >= c.ws.total;
    if (fp8 && !c.ws_ok) return LA_ERR_WORKSPACE;                                         // e4m3 cannot run without it; for bf16 / fp16 only a split needs it (below)
    if ((a->flags & LA_FLAG_LIST_INT16) && c.k_tiles + 1 > kListInt16MaxRow) return LA_ERR_SEQLEN;
    c.list_q_tiles = c.q_tiles = (a->seqlen_q + c.bm - 1) / c.bm;
    c.half_vote = uses_half_vote(a->head_dim, esize, a->flags);
    c.q_tile_begin = a->q_tile_begin; c.q_tile_count = a->q_tile_count != 0 ? a->q_tile_count : c.q_tiles;      // count 0: all (begin must then be 0)
    if (a->q_tile_count == 0 ? a->q_tile_begin != 0 : (a->q_tile_begin < 0 || a->q_tile_count < 0 || a->q_tile_begin > c.q_tiles - a->q_tile_count))
        return LA_ERR_Q_WINDOW;
    // half-vote: q-tiles (list rows) are 128-row halves, the kernel's items are pairs of them: a window starts on an even q-tile
    // and holds an even number of them unless it reaches the last one
    if (c.half_vote && a->q_tile_count != 0 && ((a->q_tile_begin & 1) || ((a->q_tile_count & 1) && a->q_tile_begin + a->q_tile_count != c.q_tiles)))
        return LA_ERR_Q_WINDOW;
    if (c.half_vote) {                                 // the kernel's geometry: items of 2 * bm rows; the lists keep bm-row rows
        c.q_tiles = (c.list_q_tiles + 1) / 2;
        c.q_tile_count = (c.q_tile_begin + c.q_tile_count + 1) / 2 - c.q_tile_begin / 2;
        c.q_tile_begin = c.q_tile_begin / 2;
    }
    const bool x64 = fp8 || !(a->flags & LA_FLAG_KERNEL_128ROW);
    if (!x64 && la::fwd_lds_bytes_v2(a->head_dim <= 128 ? a->head_dim : 256, c.k_tiles, nullptr) > la::X_LDS_LIMIT) return LA_ERR_SEQLEN;
    if (static_cast<int64_t>(a->batch) * a->num_heads * c.q_tiles > 0x7fffffffLL) return LA_ERR_SHAPE;
    // Keys too long for the walk of ONE launch of the hand-scheduled kernels. Lists name their tiles over the whole key range and keep the bound,
    // a varlen launch too; a dense launch is cut into runs (ws.split) - of every q-tile, of a V la_fwd prepares run by run (the flag means
    // nothing to bf16 / fp16), and with the workspace for the runs' partials, which bf16 / fp16 callers may have left out.
    const bool too_long = c.ws.split || (x64 && (skipable || varlen) &&
                                         la::fwd_lds_size_x64(esize, a->head_dim, c.k_tiles, c.half_vote && skipable).bytes > la::X_LDS_LIMIT);
    if (too_long && (!c.ws.split || c.q_tile_count != c.q_tiles || (fp8 && (a->flags & LA_FLAG_V_PREPARED)) || !c.ws_ok)) return LA_ERR_SEQLEN;
    return LA_OK;
}

la::FwdParams fwd_fill(const la_fwd_args* a, const FwdChecked& c, const float* thr_head, int64_t thr_bs, int64_t thr_hs) {
    la::FwdParams p{};
    p.q = static_cast<const uint16_t*>(a->q);
    p.k = static_cast<const uint16_t*>(a->k);
    p.v = static_cast<const uint16_t*>(a->v);
    p.o = static_cast<uint16_t*>(a->o);
    p.lse = a->lse;
    p.q_batch_stride = a->q_batch_stride; p.q_row_stride = a->q_row_stride; p.q_head_stride = a->q_head_stride;
    p.k_batch_stride = a->k_batch_stride; p.k_row_stride = a->k_row_stride; p.k_head_stride = a->k_head_stride;
    p.v_batch_stride = a->v_batch_stride; p.v_row_stride = a->v_row_stride; p.v_head_stride = a->v_head_stride;
    p.o_batch_stride = a->o_batch_stride; p.o_row_stride = a->o_row_stride; p.o_head_stride = a->o_head_stride;
    p.batch = a->batch; p.seqlen_q = a->seqlen_q; p.seqlen_k = a->seqlen_k; p.num_heads = a->num_heads;
    p.h_ratio = a->num_heads / a->num_heads_k;
    p.q_tiles = c.q_tiles; p.list_q_tiles = c.list_q_tiles; p.k_tiles = c.k_tiles;
    p.q_tile_begin = c.q_tile_begin; p.q_tile_count = c.q_tile_count;
    p.half_vote = c.half_vote ? 1 : 0;
    p.list_int16 = (a->flags & LA_FLAG_LIST_INT16) ? 1 : 0;
    p.scale_log2 = static_cast<float>(static_cast<double>(a->softmax_scale) * 1.4426950408889634);  // flash_api.cpp:125-126
    // softmax_scale = 0 (uniform attention: O = mean of V, LSE = ln seqlen_k) runs at c = 2^-100: every |score * c| stays far below 2^-24, so
    // each exp2 is exactly 1, while c = 0 makes NaN of the -inf of a masked key and of an empty running maximum (-inf * 0) and inf of tau / c
    if (p.scale_log2 == 0.0f) p.scale_log2 = 0x1p-100f;
    p.thr = a->thr;                                                                      // flash_api.cpp:930
    if (thr_head != nullptr && a->read_list != nullptr) { p.thr_head = thr_head; p.thr_bs = thr_bs; p.thr_hs = thr_hs; }   // (dense runs never see a table)
    p.rescale_tau = (a->flags & LA_FLAG_EXACT_RESCALE) ? 0.0f : kRescaleTauBf16;
    // the ticket block, when the workspace has it (bf16 / fp16: optional): persistent workgroups and ticket queues; without it, or under
    // LA_FLAG_STATIC_SCHED, the static one-workgroup-per-item map (same results either way)
    if (c.ws_ok && c.ws.o_part != c.ws.tickets && !(a->flags & LA_FLAG_STATIC_SCHED))
        p.work_counter = reinterpret_cast<unsigned*>(static_cast<unsigned char*>(a->workspace) + c.ws.tickets);
    p.cu_seqlens_q = a->cu_seqlens_q; p.cu_seqlens_k = a->cu_seqlens_k; p.total_q = a->total_q;
    p.read_list = a->read_list;
    p.write_list = a->write_list;
    p.must_do_list = a->must_do_list;
    p.must_do_is_1d = a->must_do_is_1d;
    p.q_descale = a->q_descale; p.k_descale = a->k_descale; p.v_descale = a->v_descale;
    p.q_descale_batch_stride = a->q_descale_batch_stride; p.q_descale_head_stride = a->q_descale_head_stride;
    p.k_descale_batch_stride = a->k_descale_batch_stride; p.k_descale_head_stride = a->k_descale_head_stride;
    p.v_descale_batch_stride = a->v_descale_batch_stride; p.v_descale_head_stride = a->v_descale_head_stride;
    return p;
}

// The runs of a split (FwdWorkspace): run s walks key rows [s, s + 1) * chunk_tiles * bn into its own contiguous partial O / LSE in the
// workspace - launch_run(ps) launches one run - then the merge by LSE writes the caller's o / lse by the caller's strides. The first error
// ends it. (The reference has no such bound: its producer reads the list from global memory, mainloop...:47-115.)
template <class LaunchRun>
hipError_t fwd_dense_runs(const la_fwd_args* a, const la::FwdParams& p, const FwdChecked& c, hipStream_t stream, LaunchRun&& launch_run) {
    const FwdWorkspace& w = c.ws;
    unsigned char* const ws = static_cast<unsigned char*>(a->workspace);
    uint16_t* const o_part = reinterpret_cast<uint16_t*>(ws + w.o_part);
    float* const lse_part = reinterpret_cast<float*>(ws + w.lse_part);
    const int64_t run_rows = static_cast<int64_t>(w.chunk_tiles) * c.bn;
    for (int s = 0; s < w.n; ++s) {
        la::FwdParams ps = p;
        const int64_t row0 = s * run_rows, left = a->seqlen_k - row0;
        ps.seqlen_k = static_cast<int>(left < run_rows ? left : run_rows);                // the last run may be shorter
        ps.k_tiles = (ps.seqlen_k + c.bn - 1) / c.bn;
        ps.k = reinterpret_cast<const uint16_t*>(static_cast<const unsigned char*>(a->k) + row0 * a->k_row_stride * c.esize);   // strides are elements
        ps.v = reinterpret_cast<const uint16_t*>(static_cast<const unsigned char*>(a->v) + row0 * a->v_row_stride * c.esize);
        ps.o = o_part + s * (w.o_bytes / 2);
        ps.o_head_stride = a->head_dim_v; ps.o_row_stride = static_cast<int64_t>(p.num_heads) * a->head_dim_v;
        ps.o_batch_stride = static_cast<int64_t>(p.seqlen_q) * ps.o_row_stride;
        ps.lse = lse_part + s * (w.lse_bytes / 4);
        const hipError_t e = launch_run(ps);
        if (e != hipSuccess) return e;
    }
    return la::launch_combine(o_part, true, c.f16, lse_part, p.o, a->lse, w.n, p.batch, p.seqlen_q, p.num_heads, a->head_dim_v, stream, false,
                              p.o_batch_stride, p.o_row_stride, p.o_head_stride);
}

// la_fwd (thr_head == nullptr) and la_fwd_head_thr: one body, so both make the same checks in the same order and fill the same block.
int fwd_run(const la_fwd_args* a, const float* thr_head, int64_t thr_bs, int64_t thr_hs, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    FwdChecked c;
    if (const int rc = fwd_check(a, c); rc != LA_OK) return rc;
    if (thr_head != nullptr) {                         // la_fwd_head_thr's own checks: behind the last of la_fwd's on every path, before the first launch
        if (a->read_list == nullptr) return LA_ERR_LISTS;                                // a dense launch votes on nothing
        if (thr_bs < 0 || thr_hs < 0 || (reinterpret_cast<uintptr_t>(thr_head) & 3u) != 0) return LA_ERR_STRIDE;
    }
    if (a->seqlen_k == 0) {
        // flash_api.cpp:1241-1245: no keys -> out = 0, lse = +inf (the write list, if any, is left as it is: nothing was walked). Varlen
        // reaches here only when EVERY sequence is empty (seqlen_k is the maximum); rows then are total_q.
        hipError_t e = c.varlen
            ? la::launch_empty_k_fill(static_cast<uint16_t*>(a->o), nullptr, 0, a->o_row_stride, a->o_head_stride, 1,
                                      static_cast<int>(a->total_q), a->num_heads, a->head_dim_v, stream)
            : la::launch_empty_k_fill(static_cast<uint16_t*>(a->o), a->lse, a->o_batch_stride, a->o_row_stride, a->o_head_stride,
                                      a->batch, a->seqlen_q, a->num_heads, a->head_dim_v, stream);
        if (e == hipSuccess && c.varlen && a->lse != nullptr && a->total_q > 0)            // +inf = 0x7f800000 is not a memset byte pattern
            e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(a->lse), 0x7f800000, static_cast<size_t>(a->total_q) * a->num_heads, stream);
        return launch_status(e);
    }
    la::FwdParams p = fwd_fill(a, c, thr_head, thr_bs, thr_hs);
    const bool skipable = a->read_list != nullptr;
    if (c.fp8) {
        // 1) V -> pre-transposed, pre-swizzled V^T tiles at the front of the workspace (split: per run ITS keys); 2) forward on (Q, K, V^T)
        const int p_mode = (a->flags & LA_FLAG_FP8_ENCODED_P) ? 0 : (a->flags & LA_FLAG_FP8_MFMA_ROWSUM) ? 1 : 2;   // default: the reference's arithmetic
        const auto launch = [&](la::FwdParams& ps, const int* cu_seqlens_k) {
            hipError_t e = hipSuccess;
            if (!(a->flags & LA_FLAG_V_PREPARED))
                e = la::launch_prep_v_fp8(ps.v, a->v_batch_stride, a->v_row_stride, a->v_head_stride, a->workspace, a->batch, ps.seqlen_k,
                                          a->num_heads_k, ps.k_tiles, a->head_dim, stream, cu_seqlens_k);
            if (e != hipSuccess) return e;
            ps.v = static_cast<const uint16_t*>(a->workspace);
            return la::launch_fwd_x64_fp8(ps, skipable, p_mode, a->head_dim, stream);
        };
        if (c.ws.split) return launch_status(fwd_dense_runs(a, p, c, stream, [&](la::FwdParams& ps) { return launch(ps, nullptr); }));
        return launch_status(launch(p, a->cu_seqlens_k));
    }
    // every instantiated head_dim: the hand-scheduled x64 kernel unless LA_FLAG_KERNEL_128ROW (the hipcc-scheduled template: 64 / 128 / 256)
    if (c.ws.split)
        return launch_status(fwd_dense_runs(a, p, c, stream, [&](la::FwdParams& ps) { return la::launch_fwd_x64(ps, a->head_dim, false, c.f16, stream); }));
    if (a->flags & LA_FLAG_KERNEL_128ROW) return launch_status(la::launch_fwd_bf16_v2(p, a->head_dim, skipable, c.f16, stream));
    return launch_status(la::launch_fwd_x64(p, a->head_dim, skipable, c.f16, stream));
}
}  // namespace

extern "C" {

int la_abi_version(void) { return LA_ABI_VERSION; }

#ifndef LA_BUILD_INFO          // liteattention_amd/build.py passes the record; a hand-run hipcc gets an honest "unknown"
#define LA_BUILD_INFO "src=unknown;variant=1;wrong_results=0;opts=built outside liteattention_amd/build.py"
#endif
#define LA_STR2(x) #x
#define LA_STR(x) LA_STR2(x)
const char* la_build_info(void) { return "abi=" LA_STR(LA_ABI_VERSION) ";" LA_BUILD_INFO; }

int la_last_hip_error(void) { return g_last_hip_error; }

const char* la_status_string(int status) {
    switch (status) {
        case LA_OK: return "ok";
        case LA_ERR_NULL_ARG: return "required pointer is NULL";
        case LA_ERR_STRUCT_SIZE: return "la_fwd_args.struct_size mismatch (ABI version skew)";
        case LA_ERR_DTYPE: return "FlashAttention only supports fp16, bf16, and fp8_e4m3 type; this build instantiates all three";
        case LA_ERR_HEAD_DIM: return "head_size not instantiated in this build (bf16 / fp16: 64, 96, 128, 192, 256 - under LA_FLAG_KERNEL_128ROW only 64, 128, 256; fp8: 64, 96, 128, 192, 256)";
        case LA_ERR_SHAPE: return "invalid shape (batch, seqlen_q, heads and head_dim must be positive; number of heads in key/value must divide number of heads in query)";
        case LA_ERR_STRIDE: return "Input tensor must have contiguous last dimension and 16-byte aligned rows (la_fwd: K / V row stride at most 2^26 bytes, Q / O row stride below 2^30 elements)";
        case LA_ERR_TILE_MISMATCH: return "block_m/block_n do not match la_get_tile_sizes(): skip lists would be mis-indexed";
        case LA_ERR_LISTS: return "attn_read_list and attn_write_list must be given together";
        case LA_ERR_UNSUPPORTED: return "feature outside the QK-Skip hot path (head_dim_v != head_dim, unknown flags, skip lists with cu_seqlens on the 128-row kernels or, for bf16 / fp16, above head_dim 128)";
        case LA_ERR_LAUNCH: return "HIP kernel launch failed (see la_last_hip_error)";
        case LA_ERR_SEQLEN: return "seqlen_k too long: the expanded skip list does not fit in LDS (dense launches are cut into runs and merged when the workspace of la_fwd_workspace_bytes() is given)";   // also: LA_FLAG_LIST_INT16 / list_elem_size 2 with k_tiles + 1 > 32767 (the message is pinned by the callers' tests)
        case LA_ERR_WORKSPACE: return "fp8 needs a 16-byte aligned workspace of la_fwd_workspace_bytes() bytes";
        case LA_ERR_Q_WINDOW: return "q_tile_begin/q_tile_count outside the q-tiles of this problem (LA_FLAG_HALF_VOTE: windows start on an even q-tile and hold an even number unless they reach the last)";
        default: return "unknown la_status";
    }
}

int la_get_tile_sizes_ex(int head_dim, int element_size, uint32_t flags, int* block_m, int* block_n) {
    la::TileShape t = la::tile_shape(head_dim, element_size);
    if (t.block_m == 0) return (element_size == 2 || element_size == 1) ? LA_ERR_HEAD_DIM : LA_ERR_DTYPE;
    if ((flags & ~kKnownFlags) != 0) return LA_ERR_UNSUPPORTED;
    if ((flags & LA_FLAG_KERNEL_128ROW) && element_size == 1) return LA_ERR_UNSUPPORTED;   // the 128-row fp8 kernel is not in this build
    if ((flags & LA_FLAG_KERNEL_128ROW) && (head_dim == 96 || head_dim == 192)) return LA_ERR_HEAD_DIM;   // the hipcc-scheduled template has 64 / 128 / 256
    if (uses_128row(head_dim, element_size, flags)) t.block_m = 128;                       // A/B kernel: 32 rows per wave
    if (uses_half_vote(head_dim, element_size, flags)) t.block_m = 128;                    // lists per 128-row half of the 256-row workgroup
    if (block_m) *block_m = t.block_m;
    if (block_n) *block_n = t.block_n;
    return LA_OK;
}

int la_get_tile_sizes(int head_dim, int element_size, int* block_m, int* block_n) {
    return la_get_tile_sizes_ex(head_dim, element_size, 0u, block_m, block_n);
}

int64_t la_fwd_workspace_bytes(const la_fwd_args* a) {
    if (a == nullptr) return LA_ERR_NULL_ARG;
    if (a->struct_size != sizeof(la_fwd_args)) return LA_ERR_STRUCT_SIZE;
    const bool fp8 = a->dtype == LA_DTYPE_FP8_E4M3;
    if (!fp8 && a->dtype != LA_DTYPE_BF16 && a->dtype != LA_DTYPE_FP16) return LA_ERR_DTYPE;
    int bm = 0, bn = 0;
    const int trc = la_get_tile_sizes_ex(a->head_dim, fp8 ? 1 : 2, fp8 ? a->flags : a->flags & kKnownFlags, &bm, &bn);
    // The two dtypes answer a block la_fwd refuses differently, and callers have seen both: e4m3 returns the code of a head dim, flag or size
    // it cannot size tiles for; bf16 / fp16 check nothing and size such a block (one without kernels or without rows; unknown flags are
    // not looked at) as ONE launch: the ticket block or nothing.
    if (fp8) {
        if (trc != LA_OK) return trc;
        if (a->batch <= 0 || a->num_heads <= 0 || a->num_heads_k <= 0 || a->seqlen_k < 0) return LA_ERR_SHAPE;
    }
    const bool may_split = fp8 ? a->seqlen_q > 0 : trc == LA_OK && a->seqlen_k > 0 && a->batch > 0 && a->seqlen_q > 0 && a->num_heads > 0;
    return static_cast<int64_t>(fwd_workspace(a, fp8 ? 1 : 2, trc == LA_OK ? (a->seqlen_k + bn - 1) / bn : 0, may_split).total);
}

int la_fwd(const la_fwd_args* a, void* stream_) { return fwd_run(a, nullptr, 0, 0, stream_); }

int la_fwd_head_thr(const la_fwd_args* a, const float* thr_head, int64_t thr_batch_stride, int64_t thr_head_stride, void* stream_) {
    return fwd_run(a, thr_head, thr_batch_stride, thr_head_stride, stream_);
}

int la_skip_list_stats_ex(const void* list, int32_t list_elem_size, int32_t n_batch, int32_t num_heads, int32_t q_tiles, int32_t k_tiles,
                          int64_t* out_counts, void* stream_) {
    if (!list || !out_counts) return LA_ERR_NULL_ARG;
    if (const int rc = list_geometry_status(list_elem_size, n_batch, num_heads, q_tiles, k_tiles); rc != LA_OK) return rc;
    const hipError_t err = la::launch_skip_list_stats(list, list_elem_size, n_batch * num_heads * q_tiles, k_tiles, out_counts,
                                                      static_cast<hipStream_t>(stream_));
    return launch_status(err);
}

int la_skip_list_stats_heads(const void* list, int32_t list_elem_size, int32_t n_batch, int32_t num_heads, int32_t q_tiles, int32_t k_tiles,
                             int64_t* out_counts, void* stream_) {
    if (!list || !out_counts) return LA_ERR_NULL_ARG;
    if (const int rc = list_geometry_status(list_elem_size, n_batch, num_heads, q_tiles, k_tiles); rc != LA_OK) return rc;
    const hipError_t err = la::launch_skip_list_stats_heads(list, list_elem_size, n_batch * num_heads, q_tiles, k_tiles, out_counts,
                                                            static_cast<hipStream_t>(stream_));
    return launch_status(err);
}

int la_skip_list_stats(const int32_t* list, int32_t n_batch, int32_t num_heads, int32_t q_tiles, int32_t k_tiles,
                       int64_t* out_counts, void* stream_) {
    return la_skip_list_stats_ex(list, 4, n_batch, num_heads, q_tiles, k_tiles, out_counts, stream_);
}

int la_blockmask_to_lists_ex(const uint8_t* blockmask, int64_t mask_batch_stride, int64_t mask_head_stride, int32_t batch,
                             int32_t num_heads, int32_t q_tiles, int32_t k_tiles, const int32_t* q_tiles_valid,
                             const int32_t* k_tiles_valid, void* lists, int32_t list_elem_size, int32_t* empty_rows, void* stream_) {
    if (!blockmask || !lists) return LA_ERR_NULL_ARG;
    if (const int rc = list_geometry_status(list_elem_size, batch, num_heads, q_tiles, k_tiles, mask_batch_stride >= 0 && mask_head_stride >= 0); rc != LA_OK)
        return rc;
    const hipError_t err = la::launch_blockmask_to_lists(blockmask, mask_batch_stride, mask_head_stride, batch, num_heads, q_tiles,
                                                         k_tiles, q_tiles_valid, k_tiles_valid, lists, list_elem_size, empty_rows,
                                                         static_cast<hipStream_t>(stream_));
    return launch_status(err);
}

int la_blockmask_to_lists(const uint8_t* blockmask, int64_t mask_batch_stride, int64_t mask_head_stride, int32_t batch,
                          int32_t num_heads, int32_t q_tiles, int32_t k_tiles, const int32_t* q_tiles_valid,
                          const int32_t* k_tiles_valid, int32_t* lists, int32_t* empty_rows, void* stream_) {
    return la_blockmask_to_lists_ex(blockmask, mask_batch_stride, mask_head_stride, batch, num_heads, q_tiles, k_tiles, q_tiles_valid,
                                    k_tiles_valid, lists, 4, empty_rows, stream_);
}

int la_device_slots(int head_dim, int element_size, uint32_t flags, int* compute_units, int* workgroups_per_cu) {
    int bm = 0, bn = 0;
    const int rc = la_get_tile_sizes_ex(head_dim, element_size, flags, &bm, &bn);
    if (rc != LA_OK) return rc;
    // the hand-scheduled kernels fill a CU with ONE workgroup (512 registers x 4 waves, 64-130 KiB of LDS; the two-waves-per-SIMD A/B body
    // of head_dim 64 is one 8-wave workgroup too); the hipcc-scheduled 128-row template runs two per CU at head_dim <= 128 (la_fwd_kernel_v2.hip)
    const bool v2 = element_size == 2 && (flags & LA_FLAG_KERNEL_128ROW) != 0;
    if (compute_units) *compute_units = la::compute_units();
    if (workgroups_per_cu) *workgroups_per_cu = v2 ? (head_dim <= 128 ? 2 : 1) : (element_size == 2 ? la::x64_workgroups_per_cu(head_dim) : 1);
    return LA_OK;
}

int la_combine(const void* o_partial, int32_t partial_is_16bit, const float* lse_partial, void* o, int32_t o_dtype, float* lse,
               int32_t num_splits, int32_t batch, int32_t seqlen_q, int32_t num_heads, int32_t head_dim_v,
               void* stream_) {
    if (!o_partial || !lse_partial || !o) return LA_ERR_NULL_ARG;
    if (const int rc = combine_status(o, o_dtype, partial_is_16bit, num_splits, 0x7fffffff, batch, seqlen_q, num_heads, head_dim_v); rc != LA_OK) return rc;
    if (!aligned16(o_partial)) return LA_ERR_STRIDE;
    const hipError_t err = la::launch_combine(o_partial, partial_is_16bit != 0, o_dtype == LA_DTYPE_FP16, lse_partial, static_cast<uint16_t*>(o), lse,
                                              num_splits, batch, seqlen_q, num_heads, head_dim_v,
                                              static_cast<hipStream_t>(stream_), o_dtype == LA_DTYPE_FP32);
    return launch_status(err);
}

int la_combine_list(const void* const* o_partials, int32_t partial_is_16bit, const float* const* lse_partials, void* o, int32_t o_dtype,
                    float* lse, int32_t num_splits, int32_t batch, int32_t seqlen_q, int32_t num_heads, int32_t head_dim_v, void* stream_) {
    if (!o_partials || !lse_partials || !o) return LA_ERR_NULL_ARG;
    if (const int rc = combine_status(o, o_dtype, partial_is_16bit, num_splits, LA_COMBINE_LIST_MAX, batch, seqlen_q, num_heads, head_dim_v); rc != LA_OK)
        return rc;
    for (int i = 0; i < num_splits; ++i) {
        if (!o_partials[i] || !lse_partials[i]) return LA_ERR_NULL_ARG;
        if (!aligned16(o_partials[i])) return LA_ERR_STRIDE;
    }
    const hipError_t err = la::launch_combine_list(o_partials, partial_is_16bit != 0, o_dtype == LA_DTYPE_FP16, lse_partials, static_cast<uint16_t*>(o),
                                                   lse, num_splits, batch, seqlen_q, num_heads, head_dim_v, static_cast<hipStream_t>(stream_),
                                                   o_dtype == LA_DTYPE_FP32);
    return launch_status(err);
}

int la_output_error(const void* out, int32_t out_dtype, int64_t out_batch_stride, int64_t out_row_stride, int64_t out_head_stride,
                    const void* ref, int32_t ref_dtype, int64_t ref_batch_stride, int64_t ref_row_stride, int64_t ref_head_stride,
                    int32_t batch, int32_t seqlen, int32_t num_heads, int32_t head_dim, int32_t rows_per_bin, double* stats, void* stream_) {
    if (!out || !ref || !stats) return LA_ERR_NULL_ARG;
    if (!is_input_dtype(out_dtype) || !is_input_dtype(ref_dtype)) return LA_ERR_DTYPE;
    if (batch <= 0 || seqlen <= 0 || num_heads <= 0 || head_dim <= 0 || rows_per_bin <= 0) return LA_ERR_SHAPE;
    if (head_dim % 8 != 0) return LA_ERR_HEAD_DIM;
    // every row start is a 16-byte boundary (rows_aligned). This entry point holds the row and the head stride to it also where seqlen or
    // num_heads is 1 and the stride goes unused - only the batch stride of batch 1 is exempt, as its header says: hence the 2s
    if (!rows_aligned(out, out_dtype, out_batch_stride, out_row_stride, out_head_stride, batch, 2, 2) ||
        !rows_aligned(ref, ref_dtype, ref_batch_stride, ref_row_stride, ref_head_stride, batch, 2, 2)) return LA_ERR_STRIDE;
    const int64_t nbins = (static_cast<int64_t>(seqlen) + rows_per_bin - 1) / rows_per_bin;
    if (static_cast<int64_t>(batch) * num_heads * nbins > 0x7fffffffLL) return LA_ERR_SHAPE;       // one workgroup per stats row
    const hipError_t err = la::launch_output_error(out, out_dtype, out_batch_stride, out_row_stride, out_head_stride, ref, ref_dtype,
                                                   ref_batch_stride, ref_row_stride, ref_head_stride, batch, seqlen, num_heads, head_dim,
                                                   rows_per_bin, stats, static_cast<hipStream_t>(stream_));
    return launch_status(err);
}

}  // extern "C"

// What la_qk_prep, la_qk_prep_fp8 and la_qk_prep_smooth check alike, from the norm mode on, and the kernel parameters they share. A: any
// of the three argument structs (the same field names). out_dtype: la_dtype of out (LA_DTYPE_FP8_E4M3: 8 elements = 8 bytes, row starts on 8-byte boundaries).
// map: the la_row_map of a _rows entry point (its struct_size already checked), NULL for the unmapped ones: x then has seqlen rows, and
// each rule of the map sits with the unmapped rules of its kind.
template <class A>
static int qk_prep_check_and_fill(const A* a, int32_t out_dtype, const la_row_map* map, la::QkPrepParams& p) {
    const int32_t src_seqlen = map ? map->src_seqlen : a->seqlen;
    if (a->norm_mode != LA_NORM_NONE && a->norm_mode != LA_NORM_TOKEN && a->norm_mode != LA_NORM_HEAD) return LA_ERR_UNSUPPORTED;
    if (a->batch <= 0 || a->seqlen <= 0 || a->num_heads <= 0 || a->head_dim <= 0) return LA_ERR_SHAPE;
    // without src_rows out row s is made from row s of x: x has at least seqlen rows
    if (map && (src_seqlen < 1 || (!map->src_rows && src_seqlen < a->seqlen))) return LA_ERR_SHAPE;
    if (a->head_dim % 8 != 0 || a->head_dim > 256) return LA_ERR_HEAD_DIM;
    // LA_NORM_TOKEN: the token stays in registers from the load to the store - of one wave up to 5120 elements, of the four waves of a
    // workgroup up to 8 chunks of 8 elements per lane
    if (a->norm_mode == LA_NORM_TOKEN && static_cast<int64_t>(a->num_heads) * a->head_dim > 16384) return LA_ERR_UNSUPPORTED;
    // every row start is aligned (rows_aligned), and the kernels keep a chunk's offset from its token's start in 32 bits
    const auto strides_ok = [&](const void* ptr, int32_t d, int64_t bs, int64_t rs, int64_t hs, int32_t rows) {
        return rows_aligned(ptr, d, bs, rs, hs, a->batch, rows, a->num_heads) && hs <= (0x7fffffffLL - a->head_dim) / a->num_heads;
    };
    if (!strides_ok(a->x, a->in_dtype, a->x_batch_stride, a->x_row_stride, a->x_head_stride, src_seqlen) ||
        (a->out && !strides_ok(a->out, out_dtype, a->out_batch_stride, a->out_row_stride, a->out_head_stride, a->seqlen))) return LA_ERR_STRIDE;
    if (map && (map->batch_stride < 0 ||
                ((reinterpret_cast<uintptr_t>(map->src_rows) | reinterpret_cast<uintptr_t>(map->positions)) & 3u))) return LA_ERR_STRIDE;
    if (map && map->src_rows && a->out == a->x) return LA_ERR_UNSUPPORTED;        // a gather in place: rows would be read after they were overwritten
    if (a->weight && !aligned16(a->weight)) return LA_ERR_STRIDE;                 // read 16 bytes at a time
    for (int i = 0; i < 3; ++i)
        if (reinterpret_cast<uintptr_t>(a->rope_table[i]) & 7u) return LA_ERR_STRIDE;      // (cos, sin) is one 8-byte load
    int64_t pairs = 0;
    for (int i = 0; i < 3; ++i) {
        if (a->axis_pairs[i] < 0) return LA_ERR_SHAPE;
        pairs += a->axis_pairs[i];
    }
    if (pairs > a->head_dim / 2) return LA_ERR_SHAPE;
    const bool rotate = a->rope_table[0] || a->rope_table[1] || a->rope_table[2];      // all three NULL: norm and cast only
    if (a->pos_offset < 0) return LA_ERR_SHAPE;
    int64_t pos_limit = 1;
    if (rotate) {
        for (int i = 0; i < 3; ++i)
            if (!a->rope_table[i] && a->axis_pairs[i] > 0) return LA_ERR_NULL_ARG;
        int64_t positions = 1;
        for (int i = 0; i < 3; ++i) {
            if (a->axis_extent[i] <= 0) return LA_ERR_SHAPE;
            positions *= a->axis_extent[i];                       // three factors below 2^31: the product of the first two fits, the third is checked
            if (i == 1 && positions > 0x7fffffffLL) return LA_ERR_SHAPE;
        }
        // the positions of a table are clamped by the kernel; without one the last position is that of x's last row
        if (positions > 0x7fffffffLL || (!(map && map->positions) && static_cast<int64_t>(a->pos_offset) + src_seqlen > positions))
            return LA_ERR_SHAPE;
        pos_limit = positions;
    }
    p = {};
    p.x = a->x; p.out = a->out; p.weight = a->norm_mode == LA_NORM_NONE ? nullptr : a->weight;
    p.x_bs = a->x_batch_stride; p.x_rs = a->x_row_stride; p.x_hs = a->x_head_stride;
    p.o_bs = a->out_batch_stride; p.o_rs = a->out_row_stride; p.o_hs = a->out_head_stride;
    p.tokens = static_cast<int64_t>(a->batch) * a->seqlen;
    p.seqlen = a->seqlen; p.num_heads = a->num_heads; p.head_dim = a->head_dim;
    p.norm_mode = a->norm_mode; p.rotate = rotate && pairs > 0 ? 1 : 0;
    p.ext1 = rotate ? a->axis_extent[1] : 1; p.ext2 = rotate ? a->axis_extent[2] : 1;
    for (int i = 0; i < 3; ++i) { p.table[i] = a->rope_table[i]; p.pairs[i] = rotate ? a->axis_pairs[i] : 0; }
    p.pos_offset = a->pos_offset; p.eps = a->eps;
    p.src_seqlen = src_seqlen; p.pos_limit = static_cast<int>(pos_limit);
    if (map) { p.src_rows = map->src_rows; p.positions = map->positions; p.map_bs = map->batch_stride; }
    return LA_OK;
}

// The scale fields, which la_qk_prep_fp8 and la_qk_prep_smooth check and fill alike, in the three places their order of checks has: the
// group size with the other shapes, the strides and pointers with the other strides, both before the shared checks ...
template <class A>
static bool qk_prep_scale_groups_ok(const A* a) {
    return a->num_heads > 0 && a->heads_per_scale >= 1 && a->num_heads % a->heads_per_scale == 0;
}
template <class A>
static bool qk_prep_scale_strides_ok(const A* a) {
    return a->descale_batch_stride >= 0 && a->descale_head_stride >= 0 && a->amax_batch_stride >= 0 && a->amax_head_stride >= 0 &&
           ((reinterpret_cast<uintptr_t>(a->descale) | reinterpret_cast<uintptr_t>(a->amax)) & 3u) == 0;
}
// ... and behind them the limit of heads and the fill, with everything shared with la_qk_prep
template <class A>
static int qk_prep_e4m3_check_and_fill(const A* a, const la_row_map* map, la::QkPrepParams& p) {
    const int rc = qk_prep_check_and_fill(a, LA_DTYPE_FP8_E4M3, map, p);
    if (rc != LA_OK) return rc;
    if (a->num_heads > la::kQkPrepScaleSlots) return LA_ERR_UNSUPPORTED;      // a workgroup keeps every head's scale and maximum in LDS
    p.descale = a->out ? a->descale : nullptr; p.amax = a->amax;
    p.ds_bs = a->descale_batch_stride; p.ds_hs = a->descale_head_stride;
    p.am_bs = a->amax_batch_stride; p.am_hs = a->amax_head_stride;
    p.heads_per_scale = a->heads_per_scale;
    return LA_OK;
}

// The three passes, each behind its unmapped entry point (mapped false, map NULL) and its _rows one (mapped true: a map is required; it is
// checked for presence with the arguments and for its size behind theirs, its fields inside the shared checker).
static bool row_map_size_ok(bool mapped, const la_row_map* map) { return !mapped || map->struct_size == sizeof(la_row_map); }

static int qk_prep_run(const la_qk_prep_args* a, bool mapped, const la_row_map* map, void* stream_) {
    if (!a || (mapped && !map)) return LA_ERR_NULL_ARG;
    if (a->struct_size != sizeof(la_qk_prep_args) || !row_map_size_ok(mapped, map)) return LA_ERR_STRUCT_SIZE;
    if (!a->x || !a->out) return LA_ERR_NULL_ARG;
    if (!is_input_dtype(a->in_dtype) || (a->out_dtype != LA_DTYPE_BF16 && a->out_dtype != LA_DTYPE_FP16)) return LA_ERR_DTYPE;
    la::QkPrepParams p;
    const int rc = qk_prep_check_and_fill(a, a->out_dtype, map, p);
    if (rc != LA_OK) return rc;
    return launch_status(la::launch_qk_prep(p, a->in_dtype, a->out_dtype, 0, static_cast<hipStream_t>(stream_)));
}

static int qk_prep_fp8_run(const la_qk_prep_fp8_args* a, bool mapped, const la_row_map* map, void* stream_) {
    if (!a || (mapped && !map)) return LA_ERR_NULL_ARG;
    if (a->struct_size != sizeof(la_qk_prep_fp8_args) || !row_map_size_ok(mapped, map)) return LA_ERR_STRUCT_SIZE;
    if (!a->x || (!a->out && !a->amax)) return LA_ERR_NULL_ARG;
    if (!is_input_dtype(a->in_dtype)) return LA_ERR_DTYPE;
    if (!qk_prep_scale_groups_ok(a)) return LA_ERR_SHAPE;
    if (!qk_prep_scale_strides_ok(a)) return LA_ERR_STRIDE;
    la::QkPrepParams p;
    const int rc = qk_prep_e4m3_check_and_fill(a, map, p);
    if (rc != LA_OK) return rc;
    return launch_status(la::launch_qk_prep(p, a->in_dtype, LA_DTYPE_FP8_E4M3, a->out ? 1 : 2, static_cast<hipStream_t>(stream_)));
}

static int qk_prep_smooth_run(const la_qk_prep_smooth_args* a, bool mapped, const la_row_map* map, void* stream_) {
    if (!a || (mapped && !map)) return LA_ERR_NULL_ARG;
    if (a->struct_size != sizeof(la_qk_prep_smooth_args) || !row_map_size_ok(mapped, map)) return LA_ERR_STRUCT_SIZE;
    if (!a->x || (!a->out && !a->amax && !a->colsum_part && !a->dot_out)) return LA_ERR_NULL_ARG;
    if ((a->dot_out != nullptr) != (a->dot_vec != nullptr)) return LA_ERR_NULL_ARG;
    if (!is_input_dtype(a->in_dtype)) return LA_ERR_DTYPE;
    if (!qk_prep_scale_groups_ok(a)) return LA_ERR_SHAPE;
    if (a->dot_vec && (a->heads_per_dot < 1 || a->num_heads % a->heads_per_dot != 0)) return LA_ERR_SHAPE;
    if (!qk_prep_scale_strides_ok(a) || (reinterpret_cast<uintptr_t>(a->dot_out) & 3u)) return LA_ERR_STRIDE;
    // shift and dot_vec rows are read 16 bytes at a time, the part sums are written so
    if ((a->shift && !rows_aligned(a->shift, LA_DTYPE_FP32, a->shift_batch_stride, 0, a->shift_head_stride, a->batch, 1, a->num_heads)) ||
        (a->dot_vec && !rows_aligned(a->dot_vec, LA_DTYPE_FP32, a->dot_vec_batch_stride, 0, a->dot_vec_head_stride, a->batch, 1,
                                     a->num_heads / a->heads_per_dot)) ||
        !aligned16(a->colsum_part)) return LA_ERR_STRIDE;
    la::QkPrepParams p;
    const int rc = qk_prep_e4m3_check_and_fill(a, map, p);
    if (rc != LA_OK) return rc;
    // a thread keeps the running sums of its columns in LDS: at most 16 chunks of 8
    if (a->colsum_part && la::qk_prep_sum_slots(p) > la::kQkPrepSumSlots) return LA_ERR_UNSUPPORTED;
    p.batch = a->batch;
    int mode = a->out ? 1 : 2;                                      // nothing added: la_qk_prep_fp8's own kernels
    if (a->shift || a->colsum_part || a->dot_vec) {
        mode += 2;
        p.shift = a->shift; p.sh_bs = a->shift_batch_stride; p.sh_hs = a->shift_head_stride;
        p.colsum_part = a->colsum_part;
        p.dot_vec = a->dot_vec; p.dv_bs = a->dot_vec_batch_stride; p.dv_hs = a->dot_vec_head_stride;
        p.heads_per_dot = a->dot_vec ? a->heads_per_dot : 1; p.dot_out = a->dot_out;
        p.part_rows = la::qk_prep_part_rows(a->seqlen); p.part_blocks = la::qk_prep_part_blocks(a->seqlen);
    }
    return launch_status(la::launch_qk_prep(p, a->in_dtype, LA_DTYPE_FP8_E4M3, mode, static_cast<hipStream_t>(stream_)));
}

extern "C" {

int la_qk_prep(const la_qk_prep_args* a, void* stream) { return qk_prep_run(a, false, nullptr, stream); }
int la_qk_prep_rows(const la_qk_prep_args* a, const la_row_map* map, void* stream) { return qk_prep_run(a, true, map, stream); }
int la_qk_prep_fp8(const la_qk_prep_fp8_args* a, void* stream) { return qk_prep_fp8_run(a, false, nullptr, stream); }
int la_qk_prep_fp8_rows(const la_qk_prep_fp8_args* a, const la_row_map* map, void* stream) { return qk_prep_fp8_run(a, true, map, stream); }
int la_qk_prep_smooth(const la_qk_prep_smooth_args* a, void* stream) { return qk_prep_smooth_run(a, false, nullptr, stream); }
int la_qk_prep_smooth_rows(const la_qk_prep_smooth_args* a, const la_row_map* map, void* stream) {
    return qk_prep_smooth_run(a, true, map, stream);
}

int la_qk_prep_smooth_parts(int32_t seqlen, int32_t num_heads, int32_t head_dim) {
    if (seqlen <= 0 || num_heads <= 0 || head_dim <= 0) return LA_ERR_SHAPE;
    return 4 * la::qk_prep_part_blocks(seqlen);                   // today a function of seqlen alone
}

int la_qk_prep_smooth_part_rows(int32_t seqlen, int32_t num_heads, int32_t head_dim) {
    if (seqlen <= 0 || num_heads <= 0 || head_dim <= 0) return LA_ERR_SHAPE;
    return la::qk_prep_part_rows(seqlen);
}

int la_colsum_finish(const float* part, int32_t n_parts, int32_t batch, int32_t num_heads, int32_t head_dim, int32_t seqlen,
                     float* mean_out, int64_t mean_batch_stride, int64_t mean_head_stride, void* stream_) {
    if (!part || !mean_out) return LA_ERR_NULL_ARG;
    if (n_parts <= 0 || batch <= 0 || num_heads <= 0 || head_dim <= 0 || seqlen <= 0) return LA_ERR_SHAPE;
    if (mean_batch_stride < 0 || mean_head_stride < 0 || ((reinterpret_cast<uintptr_t>(part) | reinterpret_cast<uintptr_t>(mean_out)) & 3u))
        return LA_ERR_STRIDE;
    if (static_cast<int64_t>(batch) * num_heads * head_dim > 0x7fffffffLL * 256) return LA_ERR_SHAPE;      // one thread per column
    const hipError_t err = la::launch_colsum_finish(part, n_parts, batch, num_heads, head_dim, seqlen, mean_out, mean_batch_stride,
                                                    mean_head_stride, static_cast<hipStream_t>(stream_));
    return launch_status(err);
}

// ---- V smoothing (la_prep_v.hip) ---------------------------------------------------------------------------------------------------
int la_v_colstats_parts(int32_t seqlen, int32_t num_heads, int32_t head_dim) {
    if (seqlen <= 0 || num_heads <= 0 || head_dim <= 0) return LA_ERR_SHAPE;
    return la::v_colstats_parts(seqlen, num_heads, head_dim);
}

int la_v_colstats_part_rows(int32_t seqlen, int32_t num_heads, int32_t head_dim) {
    if (seqlen <= 0 || num_heads <= 0 || head_dim <= 0) return LA_ERR_SHAPE;
    return la::v_colstats_part_rows(seqlen, num_heads, head_dim);
}

int la_v_colstats(const la_v_colstats_args* a, void* stream_) {
    if (!a) return LA_ERR_NULL_ARG;
    if (a->struct_size != sizeof(la_v_colstats_args)) return LA_ERR_STRUCT_SIZE;
    if (!a->x || !a->stat_part) return LA_ERR_NULL_ARG;
    if (!is_input_dtype(a->in_dtype)) return LA_ERR_DTYPE;
    if (a->batch <= 0 || a->seqlen <= 0 || a->num_heads <= 0 || a->head_dim <= 0) return LA_ERR_SHAPE;
    if (a->head_dim % 8 != 0 || a->head_dim > 256) return LA_ERR_HEAD_DIM;
    if (!rows_aligned(a->x, a->in_dtype, a->x_batch_stride, a->x_row_stride, a->x_head_stride, a->batch, a->seqlen, a->num_heads) ||
        !aligned16(a->stat_part)) return LA_ERR_STRIDE;
    la::VColstatsParams p = {};
    p.x = a->x; p.stat_part = a->stat_part;
    p.x_bs = a->x_batch_stride; p.x_rs = a->x_row_stride; p.x_hs = a->x_head_stride;
    p.batch = a->batch; p.seqlen = a->seqlen; p.num_heads = a->num_heads; p.head_dim = a->head_dim;
    p.n_parts = la::v_colstats_parts(a->seqlen, a->num_heads, a->head_dim);
    p.part_rows = la::v_colstats_part_rows(a->seqlen, a->num_heads, a->head_dim);
    // one thread per (part, batch, head, chunk of 8 columns), 256 per workgroup
    if (static_cast<int64_t>(p.n_parts) * a->batch * a->num_heads * (a->head_dim / 8) > 0x7fffffffLL * 256) return LA_ERR_SHAPE;
    const hipError_t err = la::launch_v_colstats(p, a->in_dtype, static_cast<hipStream_t>(stream_));
    return launch_status(err);
}

int la_v_colstats_finish(const float* part, int32_t n_parts, int32_t batch, int32_t num_heads, int32_t head_dim, int32_t seqlen,
                         float* mean_out, int64_t mean_batch_stride, int64_t mean_head_stride, float* amax_out, int64_t amax_batch_stride,
                         int64_t amax_head_stride, void* stream_) {
    if (!part || !mean_out) return LA_ERR_NULL_ARG;
    if (n_parts <= 0 || batch <= 0 || num_heads <= 0 || head_dim <= 0 || seqlen <= 0) return LA_ERR_SHAPE;
    if (head_dim > 256) return LA_ERR_HEAD_DIM;                                   // one thread of a workgroup per column of a head
    if (mean_batch_stride < 0 || mean_head_stride < 0 || amax_batch_stride < 0 || amax_head_stride < 0 ||
        ((reinterpret_cast<uintptr_t>(part) | reinterpret_cast<uintptr_t>(mean_out) | reinterpret_cast<uintptr_t>(amax_out)) & 3u))
        return LA_ERR_STRIDE;
    if (static_cast<int64_t>(batch) * num_heads > 0x7fffffffLL) return LA_ERR_SHAPE;                       // one workgroup per head
    const hipError_t err = la::launch_v_colstats_finish(part, n_parts, batch, num_heads, head_dim, seqlen, mean_out, mean_batch_stride,
                                                        mean_head_stride, amax_out, amax_batch_stride, amax_head_stride,
                                                        static_cast<hipStream_t>(stream_));
    return launch_status(err);
}

int la_attn_unshift(const la_attn_unshift_args* a, void* stream_) {
    if (!a) return LA_ERR_NULL_ARG;
    if (a->struct_size != sizeof(la_attn_unshift_args)) return LA_ERR_STRUCT_SIZE;
    if (!a->o || !a->out) return LA_ERR_NULL_ARG;
    if ((a->lse_dot != nullptr) != (a->lse_out != nullptr) || (a->lse_out && !a->lse)) return LA_ERR_NULL_ARG;
    if (a->o_dtype != LA_DTYPE_BF16 && a->o_dtype != LA_DTYPE_FP16) return LA_ERR_DTYPE;
    if (!is_input_dtype(a->out_dtype)) return LA_ERR_DTYPE;
    if (a->batch <= 0 || a->seqlen <= 0 || a->num_heads <= 0 || a->head_dim <= 0) return LA_ERR_SHAPE;
    if (a->shift && (a->heads_per_vec < 1 || a->num_heads % a->heads_per_vec != 0)) return LA_ERR_SHAPE;
    if (a->head_dim % 8 != 0) return LA_ERR_HEAD_DIM;
    if (!rows_aligned(a->o, a->o_dtype, a->o_batch_stride, a->o_row_stride, a->o_head_stride, a->batch, a->seqlen, a->num_heads) ||
        !rows_aligned(a->out, a->out_dtype, a->out_batch_stride, a->out_row_stride, a->out_head_stride, a->batch, a->seqlen, a->num_heads))
        return LA_ERR_STRIDE;
    if (a->shift && !rows_aligned(a->shift, LA_DTYPE_FP32, a->shift_batch_stride, 0, a->shift_head_stride, a->batch, 1,
                            a->num_heads / a->heads_per_vec)) return LA_ERR_STRIDE;
    if ((reinterpret_cast<uintptr_t>(a->lse) | reinterpret_cast<uintptr_t>(a->lse_dot) | reinterpret_cast<uintptr_t>(a->lse_out)) & 3u)
        return LA_ERR_STRIDE;
    la::AttnUnshiftParams p = {};
    p.o = a->o; p.out = a->out; p.shift = a->shift; p.lse = a->lse; p.lse_dot = a->lse_dot; p.lse_out = a->lse_out;
    p.o_bs = a->o_batch_stride; p.o_rs = a->o_row_stride; p.o_hs = a->o_head_stride;
    p.out_bs = a->out_batch_stride; p.out_rs = a->out_row_stride; p.out_hs = a->out_head_stride;
    p.sh_bs = a->shift_batch_stride; p.sh_hs = a->shift_head_stride;
    p.batch = a->batch; p.seqlen = a->seqlen; p.num_heads = a->num_heads; p.head_dim = a->head_dim;
    p.heads_per_vec = a->shift ? a->heads_per_vec : 1;
    p.softmax_scale = a->softmax_scale;
    const hipError_t err = la::launch_attn_unshift(p, a->o_dtype, a->out_dtype, static_cast<hipStream_t>(stream_));
    return launch_status(err);
}

int la_attn_unshift_fp8(const la_attn_unshift_fp8_args* a, void* stream_) {
    if (!a) return LA_ERR_NULL_ARG;
    if (a->struct_size != sizeof(la_attn_unshift_fp8_args)) return LA_ERR_STRUCT_SIZE;
    if (!a->o || !a->out || (!a->descale_in && !a->row_descale)) return LA_ERR_NULL_ARG;
    if ((a->lse_dot != nullptr) != (a->lse_out != nullptr) || (a->lse_out && !a->lse)) return LA_ERR_NULL_ARG;
    if (a->o_dtype != LA_DTYPE_BF16 && a->o_dtype != LA_DTYPE_FP16) return LA_ERR_DTYPE;
    if (a->batch <= 0 || a->seqlen <= 0 || a->num_heads <= 0 || a->head_dim <= 0) return LA_ERR_SHAPE;
    if (a->shift && (a->heads_per_vec < 1 || a->num_heads % a->heads_per_vec != 0)) return LA_ERR_SHAPE;
    if (a->heads_per_scale < 1 || a->num_heads % a->heads_per_scale != 0) return LA_ERR_SHAPE;
    if (a->head_dim % 8 != 0) return LA_ERR_HEAD_DIM;
    if (!rows_aligned(a->o, a->o_dtype, a->o_batch_stride, a->o_row_stride, a->o_head_stride, a->batch, a->seqlen, a->num_heads) ||
        !rows_aligned(a->out, LA_DTYPE_FP8_E4M3, a->out_batch_stride, a->out_row_stride, a->out_head_stride, a->batch, a->seqlen,
                      a->num_heads)) return LA_ERR_STRIDE;
    if (a->shift && !rows_aligned(a->shift, LA_DTYPE_FP32, a->shift_batch_stride, 0, a->shift_head_stride, a->batch, 1,
                            a->num_heads / a->heads_per_vec)) return LA_ERR_STRIDE;
    if ((reinterpret_cast<uintptr_t>(a->lse) | reinterpret_cast<uintptr_t>(a->lse_dot) | reinterpret_cast<uintptr_t>(a->lse_out) |
         reinterpret_cast<uintptr_t>(a->row_descale) | reinterpret_cast<uintptr_t>(a->descale_in) | reinterpret_cast<uintptr_t>(a->amax)) & 3u)
        return LA_ERR_STRIDE;
    if (a->row_descale_batch_stride < 0 || a->row_descale_row_stride < 0 || a->row_descale_group_stride < 0 ||
        a->descale_in_batch_stride < 0 || a->amax_batch_stride < 0) return LA_ERR_STRIDE;
    if (a->out == a->o) return LA_ERR_UNSUPPORTED;                   // one byte for two: a chunk's bytes lie over another chunk's elements
    // a wave keeps a scale group in registers; a workgroup the empty-row flags of every head of its rows in LDS
    if (static_cast<int64_t>(a->heads_per_scale) * a->head_dim > la::kAttnOutFp8MaxGroup || a->num_heads > la::kAttnOutFp8MaxHeads)
        return LA_ERR_UNSUPPORTED;
    // one workgroup per tile of rows of a batch
    if (static_cast<int64_t>(a->batch) * ((static_cast<int64_t>(a->seqlen) + la::kAttnOutFp8Rows - 1) / la::kAttnOutFp8Rows) > 0x7fffffffLL)
        return LA_ERR_SHAPE;
    la::AttnUnshiftParams p = {};
    p.o = a->o; p.out = a->out; p.shift = a->shift; p.lse = a->lse; p.lse_dot = a->lse_dot; p.lse_out = a->lse_out;
    p.o_bs = a->o_batch_stride; p.o_rs = a->o_row_stride; p.o_hs = a->o_head_stride;
    p.out_bs = a->out_batch_stride; p.out_rs = a->out_row_stride; p.out_hs = a->out_head_stride;
    p.sh_bs = a->shift_batch_stride; p.sh_hs = a->shift_head_stride;
    p.batch = a->batch; p.seqlen = a->seqlen; p.num_heads = a->num_heads; p.head_dim = a->head_dim;
    p.heads_per_vec = a->shift ? a->heads_per_vec : 1;
    p.softmax_scale = a->softmax_scale;
    p.heads_per_scale = a->heads_per_scale;
    if (a->descale_in) {                                             // static: the batch's scale, an optional running maximum
        p.descale_in = a->descale_in; p.di_bs = a->descale_in_batch_stride;
        p.amax = a->amax; p.am_bs = a->amax_batch_stride;
    } else {                                                         // dynamic: a scale per (token, group), written
        p.row_descale = a->row_descale;
        p.rd_bs = a->row_descale_batch_stride; p.rd_rs = a->row_descale_row_stride; p.rd_gs = a->row_descale_group_stride;
    }
    return launch_status(la::launch_attn_unshift(p, a->o_dtype, LA_DTYPE_FP8_E4M3, static_cast<hipStream_t>(stream_)));
}

// ---- fp8 V in one pass (la_prep_fp8.hip) -------------------------------------------------------------------------------------------
int64_t la_v_tiles_bytes(int32_t batch, int32_t num_heads_k, int32_t seqlen_k, int32_t head_dim) {
    if (batch <= 0 || num_heads_k <= 0 || seqlen_k < 0) return LA_ERR_SHAPE;
    if (la::tile_shape(head_dim, 1).block_m == 0) return LA_ERR_HEAD_DIM;
    return static_cast<int64_t>(la::fp8_workspace_bytes(batch, num_heads_k, (seqlen_k + 63) / 64, head_dim));
}

int64_t la_v_tiles_workspace_bytes(int32_t batch, int32_t num_heads_k, int32_t seqlen_k, int32_t head_dim) {
    const int64_t tiles = la_v_tiles_bytes(batch, num_heads_k, seqlen_k, head_dim);
    return tiles < 0 ? tiles : tiles + static_cast<int64_t>(kSchedWorkspaceBytes);      // FwdWorkspace's first two terms: an e4m3 la_fwd that is one launch
}

int la_v_prep_tiles(const la_v_prep_tiles_args* a, void* stream_) {
    if (!a) return LA_ERR_NULL_ARG;
    if (a->struct_size != sizeof(la_v_prep_tiles_args)) return LA_ERR_STRUCT_SIZE;
    if (!a->x || !a->tiles) return LA_ERR_NULL_ARG;
    if (!is_input_dtype(a->in_dtype)) return LA_ERR_DTYPE;
    if (a->batch <= 0 || a->seqlen <= 0 || a->num_heads <= 0 || a->head_dim <= 0) return LA_ERR_SHAPE;
    if (la::tile_shape(a->head_dim, 1).block_m == 0) return LA_ERR_HEAD_DIM;     // the head dims the e4m3 forward has
    if (a->reserved0 != 0) return LA_ERR_UNSUPPORTED;
    if (!rows_aligned(a->x, a->in_dtype, a->x_batch_stride, a->x_row_stride, a->x_head_stride, a->batch, a->seqlen, a->num_heads) ||
        (a->shift && !rows_aligned(a->shift, LA_DTYPE_FP32, a->shift_batch_stride, 0, a->shift_head_stride, a->batch, 1, a->num_heads)) ||
        !aligned16(a->tiles) || a->descale_batch_stride < 0 || a->descale_head_stride < 0 || a->amax_batch_stride < 0 ||
        a->amax_head_stride < 0 || ((reinterpret_cast<uintptr_t>(a->descale) | reinterpret_cast<uintptr_t>(a->amax)) & 3u))
        return LA_ERR_STRIDE;
    la::VPrepTilesParams p = {};
    p.k_tiles = (a->seqlen + 63) / 64;
    if (static_cast<int64_t>(a->batch) * a->num_heads * p.k_tiles > 0x7fffffffLL) return LA_ERR_SHAPE;      // one workgroup per tile
    p.x = a->x; p.tiles = static_cast<uint8_t*>(a->tiles); p.descale = a->descale; p.shift = a->shift; p.amax = a->amax;
    p.x_bs = a->x_batch_stride; p.x_rs = a->x_row_stride; p.x_hs = a->x_head_stride;
    p.ds_bs = a->descale_batch_stride; p.ds_hs = a->descale_head_stride;
    p.sh_bs = a->shift_batch_stride; p.sh_hs = a->shift_head_stride;
    p.am_bs = a->amax_batch_stride; p.am_hs = a->amax_head_stride;
    p.batch = a->batch; p.seqlen = a->seqlen; p.num_heads = a->num_heads; p.head_dim = a->head_dim;
    return launch_status(la::launch_v_prep_tiles(p, a->in_dtype, static_cast<hipStream_t>(stream_)));
}

}  // extern "C"
