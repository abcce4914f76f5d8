// recorder.cpp - a CPU recording of what the C-ABI (liteattention_amd/csrc/la_api.hip) launches.
//
// la_api.hip holds no device code: compiled host-only it leaves undefined only the la::launch_* functions, a few size helpers and
// hipMemsetD32Async. This program supplies stand-ins for all of them, links with that object and runs on a machine without a GPU:
//   hipcc --offload-host-only -x hip -std=c++17 -I include -I liteattention_amd/csrc tests/cabi_launches/recorder.cpp \
//         liteattention_amd/csrc/la_api.hip -o recorder
// A launcher stand-in appends one record to the current case: its name, every scalar argument and every field of the parameter struct
// it was given. Pointers are fixed fake addresses, never dereferenced, printed in hex: a moved offset is a moved number. The program
// prints JSON (tests/golden/cabi_launches.json holds one digest per case of it; tests/test_cabi_launches_cpu.py compares): per case the return code,
// la_last_hip_error() (per thread and sticky: it keeps the last failed launch of EARLIER cases too), for la_fwd blocks the answer of
// la_fwd_workspace_bytes for the same block, and the ordered launch records. "legend" names the positions of every record.
//
// The size helpers (fwd_lds_bytes_v2, fp8_workspace_bytes, qk_prep_sum_slots, x64_workgroups_per_cu, compute_units) are RESTATED here or
// return what a case sets: the recorder pins what la_api.hip does with their answers, NOT the helpers. The real ones are pinned
// elsewhere: tests/test_walk_bound_cpu.py (the LDS bound and the workspace bytes, through the built library), tests/test_v_tiles_cpu.py,
// tests/test_qk_prep_smooth_cpu.py.
//
// Every case name says which check or path of la_api.hip it reaches (the first failing check decides the code: each error case is
// valid up to that check). `recorder --time N` prints the host nanoseconds of one la_fwd call (stand-in launchers that do nothing).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <chrono>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "lite_attention_amd.h"
#include "la_kernel_params.h"

namespace {
std::vector<std::string> g_launches;      // the records of the current case
std::map<std::string, std::string> g_legend;
int g_call_no = 0;                        // launcher calls of the current case so far
int g_fail_at = -1;                       // the call (0-based) that fails with g_fail_err
hipError_t g_fail_err = hipErrorInvalidValue;
long g_lds_v2 = -1;                       // >= 0: what fwd_lds_bytes_v2 answers
int g_sum_slots = -1;                     // >= 0: what qk_prep_sum_slots answers
bool g_timing = false;                    // --time: the stand-ins record nothing

std::string val(float v) { char b[48]; snprintf(b, sizeof b, "%.9g", static_cast<double>(v)); return b; }
std::string val(bool v) { return v ? "1" : "0"; }
std::string val(int v) { return std::to_string(v); }
std::string val(unsigned v) { return std::to_string(v); }
std::string val(long v) { return std::to_string(v); }
std::string val(long long v) { return std::to_string(v); }
std::string val(unsigned long v) { return std::to_string(v); }
std::string val(const void* p) { char b[32]; snprintf(b, sizeof b, "\"0x%llx\"", static_cast<unsigned long long>(reinterpret_cast<uintptr_t>(p))); return b; }
std::string val(hipStream_t p) { return val(static_cast<const void*>(p)); }

#define LA_FWD_FIELDS(X) X(q) X(k) X(v) X(o) X(lse) X(q_batch_stride) X(q_row_stride) X(q_head_stride) X(k_batch_stride) X(k_row_stride) \
    X(k_head_stride) X(v_batch_stride) X(v_row_stride) X(v_head_stride) X(o_batch_stride) X(o_row_stride) X(o_head_stride) X(batch) \
    X(seqlen_q) X(seqlen_k) X(num_heads) X(h_ratio) X(q_tiles) X(k_tiles) X(q_tile_begin) X(q_tile_count) X(list_q_tiles) X(half_vote) \
    X(seq_cap) X(walk_buffers) X(scale_log2) X(rescale_tau) X(thr) X(work_counter) X(read_list) X(write_list) X(must_do_list) \
    X(must_do_is_1d) X(q_descale) X(k_descale) X(v_descale) X(q_descale_batch_stride) X(q_descale_head_stride) \
    X(k_descale_batch_stride) X(k_descale_head_stride) X(v_descale_batch_stride) X(v_descale_head_stride) X(cu_seqlens_q) \
    X(cu_seqlens_k) X(thr_head) X(thr_bs) X(thr_hs) X(total_q) X(list_int16)
#define LA_QKPREP_FIELDS(X) X(x) X(out) X(weight) X(table[0]) X(table[1]) X(table[2]) X(x_bs) X(x_rs) X(x_hs) X(o_bs) X(o_rs) X(o_hs) \
    X(tokens) X(seqlen) X(num_heads) X(head_dim) X(norm_mode) X(rotate) X(ext1) X(ext2) X(pairs[0]) X(pairs[1]) X(pairs[2]) \
    X(pos_offset) X(eps) X(descale) X(amax) X(ds_bs) X(ds_hs) X(am_bs) X(am_hs) X(heads_per_scale) X(shift) X(colsum_part) X(dot_vec) \
    X(dot_out) X(sh_bs) X(sh_hs) X(dv_bs) X(dv_hs) X(heads_per_dot) X(batch) X(part_rows) X(part_blocks)
#define LA_VPREP_FIELDS(X) X(x) X(tiles) X(descale) X(shift) X(amax) X(x_bs) X(x_rs) X(x_hs) X(ds_bs) X(ds_hs) X(sh_bs) X(sh_hs) \
    X(am_bs) X(am_hs) X(batch) X(seqlen) X(num_heads) X(head_dim) X(k_tiles)
#define LA_VCOL_FIELDS(X) X(x) X(stat_part) X(x_bs) X(x_rs) X(x_hs) X(batch) X(seqlen) X(num_heads) X(head_dim) X(n_parts) X(part_rows)
#define LA_UNSHIFT_FIELDS(X) X(o) X(out) X(shift) X(lse) X(lse_dot) X(lse_out) X(o_bs) X(o_rs) X(o_hs) X(out_bs) X(out_rs) X(out_hs) \
    X(sh_bs) X(sh_hs) X(batch) X(seqlen) X(num_heads) X(head_dim) X(heads_per_vec) X(softmax_scale)
#define LA_VAL(f) s += val(p.f); s += ',';
#define LA_NAME(f) #f ","
#define LA_STRUCT_VAL(T, FIELDS)                                                          \
    std::string val(const la::T& p) {                                                     \
        g_legend[#T] = FIELDS(LA_NAME);                                                   \
        std::string s = "[";                                                              \
        FIELDS(LA_VAL)                                                                    \
        s.back() = ']';                                                                   \
        return s;                                                                         \
    }
LA_STRUCT_VAL(FwdParams, LA_FWD_FIELDS)
LA_STRUCT_VAL(QkPrepParams, LA_QKPREP_FIELDS)
LA_STRUCT_VAL(VPrepTilesParams, LA_VPREP_FIELDS)
LA_STRUCT_VAL(VColstatsParams, LA_VCOL_FIELDS)
LA_STRUCT_VAL(AttnUnshiftParams, LA_UNSHIFT_FIELDS)

template <class... A>
hipError_t record(const char* name, const char* arg_names, const A&... a) {
    if (g_timing) return hipSuccess;
    g_legend[name] = arg_names;
    std::string s = std::string("[\"") + name + "\"";
    ((s += "," + val(a)), ...);
    g_launches.push_back(s + "]");
    return g_call_no++ == g_fail_at ? g_fail_err : hipSuccess;
}
#define REC(name, ...) record(name, #__VA_ARGS__, __VA_ARGS__)
}  // namespace

// ---- the stand-ins: every symbol la_api.hip leaves undefined ------------------------------------------------------------------------
namespace la {
int compute_units() { return 256; }                                          // (the real one asks the device)
int x64_workgroups_per_cu(int) { return 1; }
size_t fwd_lds_bytes_v2(int head_dim, int k_tiles, int* seq_cap_out) {        // la_fwd_kernel_v2.hip, restated (or the case's value)
    const int seq_cap = (k_tiles + 3) & ~3;
    if (seq_cap_out) *seq_cap_out = seq_cap;
    if (g_lds_v2 >= 0) return static_cast<size_t>(g_lds_v2);
    return 4 * size_t(64) * head_dim * 2 + 16 + size_t(seq_cap) * 4 + 2 * size_t((k_tiles + 31) / 32) * 4 + 16;
}
size_t fp8_workspace_bytes(int batch, int num_heads, int k_tiles, int head_dim) {      // la_prep_fp8.hip, restated
    return static_cast<size_t>(batch) * num_heads * k_tiles * 64 * (head_dim == 96 ? 128 : head_dim);
}
int qk_prep_sum_slots(const QkPrepParams&) { return g_sum_slots >= 0 ? g_sum_slots : 1; }
hipError_t launch_fwd_bf16_v2(const FwdParams& p, int head_dim, bool skipable, bool f16, hipStream_t stream) {
    return REC("launch_fwd_bf16_v2", p, head_dim, skipable, f16, stream);
}
hipError_t launch_fwd_x64(const FwdParams& p, int head_dim, bool skipable, bool f16, hipStream_t stream) {
    return REC("launch_fwd_x64", p, head_dim, skipable, f16, stream);
}
hipError_t launch_fwd_x64_fp8(const FwdParams& p, bool skipable, int p_mode, int head_dim, hipStream_t stream) {
    return REC("launch_fwd_x64_fp8", p, skipable, p_mode, head_dim, stream);
}
hipError_t launch_prep_v_fp8(const void* v, int64_t v_batch_stride, int64_t v_row_stride, int64_t v_head_stride, void* vt, int batch,
                             int seqlen_k, int num_heads_k, int k_tiles, int head_dim, hipStream_t stream, const int* cu_seqlens_k) {
    return REC("launch_prep_v_fp8", v, v_batch_stride, v_row_stride, v_head_stride, vt, batch, seqlen_k, num_heads_k, k_tiles, head_dim,
               stream, cu_seqlens_k);
}
hipError_t launch_v_prep_tiles(const VPrepTilesParams& p, int in_dtype, hipStream_t stream) { return REC("launch_v_prep_tiles", p, in_dtype, stream); }
hipError_t launch_empty_k_fill(uint16_t* o, float* lse, int64_t o_batch_stride, int64_t o_row_stride, int64_t o_head_stride, int batch,
                               int seqlen_q, int num_heads, int head_dim_v, hipStream_t stream) {
    return REC("launch_empty_k_fill", o, lse, o_batch_stride, o_row_stride, o_head_stride, batch, seqlen_q, num_heads, head_dim_v, stream);
}
hipError_t launch_skip_list_stats(const void* list, int list_elem_size, int rows, int k_tiles, int64_t* out, hipStream_t stream) {
    return REC("launch_skip_list_stats", list, list_elem_size, rows, k_tiles, out, stream);
}
hipError_t launch_skip_list_stats_heads(const void* list, int list_elem_size, int heads, int q_tiles, int k_tiles, int64_t* out, hipStream_t stream) {
    return REC("launch_skip_list_stats_heads", list, list_elem_size, heads, q_tiles, k_tiles, out, stream);
}
hipError_t launch_blockmask_to_lists(const uint8_t* mask, int64_t mask_batch_stride, int64_t mask_head_stride, int batch, int num_heads,
                                     int q_tiles, int k_tiles, const int32_t* q_tiles_valid, const int32_t* k_tiles_valid, void* lists,
                                     int list_elem_size, int32_t* empty_rows, hipStream_t stream) {
    return REC("launch_blockmask_to_lists", mask, mask_batch_stride, mask_head_stride, batch, num_heads, q_tiles, k_tiles, q_tiles_valid,
               k_tiles_valid, lists, list_elem_size, empty_rows, stream);
}
hipError_t launch_combine(const void* o_partial, bool partial_is_16bit, bool f16, const float* lse_partial, uint16_t* o, float* lse,
                          int num_splits, int batch, int seqlen_q, int num_heads, int head_dim_v, hipStream_t stream, bool out_f32,
                          int64_t o_batch_stride, int64_t o_row_stride, int64_t o_head_stride) {
    return REC("launch_combine", o_partial, partial_is_16bit, f16, lse_partial, o, lse, num_splits, batch, seqlen_q, num_heads, head_dim_v,
               stream, out_f32, o_batch_stride, o_row_stride, o_head_stride);
}
hipError_t launch_combine_list(const void* const* o_partials, bool partial_is_16bit, bool f16, const float* const* lse_partials, uint16_t* o,
                               float* lse, int num_splits, int batch, int seqlen_q, int num_heads, int head_dim_v, hipStream_t stream,
                               bool out_f32) {
    std::string parts = "[";                       // the HOST arrays of device pointers: their entries, not their own addresses
    for (int i = 0; i < num_splits; ++i) parts += val(o_partials[i]) + "," + val(static_cast<const void*>(lse_partials[i])) + (i + 1 < num_splits ? "," : "");
    g_launches.push_back("[\"combine_list_partials\"," + parts + "]]");
    return REC("launch_combine_list", partial_is_16bit, f16, o, lse, num_splits, batch, seqlen_q, num_heads, head_dim_v, stream, out_f32);
}
hipError_t launch_output_error(const void* out, int out_dtype, int64_t o_bs, int64_t o_rs, int64_t o_hs, const void* ref, int ref_dtype,
                               int64_t r_bs, int64_t r_rs, int64_t r_hs, int batch, int seqlen, int num_heads, int head_dim, int rows_per_bin,
                               double* stats, hipStream_t stream) {
    return REC("launch_output_error", out, out_dtype, o_bs, o_rs, o_hs, ref, ref_dtype, r_bs, r_rs, r_hs, batch, seqlen, num_heads, head_dim,
               rows_per_bin, stats, stream);
}
hipError_t launch_qk_prep(const QkPrepParams& p, int in_dtype, int out_dtype, int mode, hipStream_t stream) {
    return REC("launch_qk_prep", p, in_dtype, out_dtype, mode, stream);
}
hipError_t launch_colsum_finish(const float* part, int n_parts, int batch, int num_heads, int head_dim, int seqlen, float* mean, int64_t m_bs,
                                int64_t m_hs, hipStream_t stream) {
    return REC("launch_colsum_finish", part, n_parts, batch, num_heads, head_dim, seqlen, mean, m_bs, m_hs, stream);
}
hipError_t launch_v_colstats(const VColstatsParams& p, int in_dtype, hipStream_t stream) { return REC("launch_v_colstats", p, in_dtype, stream); }
hipError_t launch_v_colstats_finish(const float* part, int n_parts, int batch, int num_heads, int head_dim, int seqlen, float* mean,
                                    int64_t m_bs, int64_t m_hs, float* amax, int64_t a_bs, int64_t a_hs, hipStream_t stream) {
    return REC("launch_v_colstats_finish", part, n_parts, batch, num_heads, head_dim, seqlen, mean, m_bs, m_hs, amax, a_bs, a_hs, stream);
}
hipError_t launch_attn_unshift(const AttnUnshiftParams& p, int o_dtype, int out_dtype, hipStream_t stream) {
    return REC("launch_attn_unshift", p, o_dtype, out_dtype, stream);
}
}  // namespace la
extern "C" hipError_t hipMemsetD32Async(hipDeviceptr_t dst, int value, size_t count, hipStream_t stream) {
    const void* const dst_ptr = dst;
    return REC("hipMemsetD32Async", dst_ptr, value, count, stream);
}

// ---- the cases ---------------------------------------------------------------------------------------------------------------------
namespace {
template <class T> T* fake(uintptr_t a) { return reinterpret_cast<T*>(a); }
void* const STREAM = fake<void>(0x5717ea00);
constexpr uintptr_t Q = 0x10000000, K = 0x20000000, V = 0x30000000, O = 0x40000000, LSE = 0x50000000, WS = 0x60000000, RL = 0x70000000,
                    WL = 0x71000000, MD = 0x72000000, CUQ = 0x73000000, CUK = 0x74000000, QD = 0x75000000, KD = 0x76000000, VD = 0x77000000,
                    THR = 0x78000000, X = 0x11000000, OUT = 0x41000000;
constexpr int BF16 = LA_DTYPE_BF16, FP16 = LA_DTYPE_FP16, E4M3 = LA_DTYPE_FP8_E4M3, FP32 = LA_DTYPE_FP32;
bool g_first_case = true;

struct Knobs { int fail_at = -1; hipError_t fail_err = hipErrorInvalidValue; long lds_v2 = -1; int sum_slots = -1; };

// one case: run `call`, print its code, the sticky HIP error and what it launched (`extra`: further members of the case's object)
void run_case(const std::string& name, const std::function<int64_t()>& call, const Knobs& kn = {}, const std::string& extra = "") {
    g_launches.clear();
    g_call_no = 0; g_fail_at = kn.fail_at; g_fail_err = kn.fail_err; g_lds_v2 = kn.lds_v2; g_sum_slots = kn.sum_slots;
    const int64_t rc = call();
    g_fail_at = -1; g_lds_v2 = -1; g_sum_slots = -1;
    printf("%s\n{\"name\":\"%s\",\"rc\":%lld,\"hip\":%d%s,\"launches\":[", g_first_case ? "" : ",", name.c_str(), static_cast<long long>(rc),
           la_last_hip_error(), extra.c_str());
    g_first_case = false;
    for (size_t i = 0; i < g_launches.size(); ++i) printf("%s\n  %s", i ? "," : "", g_launches[i].c_str());
    printf("]}");
}

struct Thr { const float* table = nullptr; int64_t bs = 0, hs = 0; bool head_thr = false; };
Thr table(uintptr_t addr = THR, int64_t bs = 4, int64_t hs = 1) { return {fake<const float>(addr), bs, hs, true}; }

void fwd_case(const std::string& name, const la_fwd_args* a, const Knobs& kn = {}, const Thr& t = {}) {
    const std::string ws = ",\"ws\":" + std::to_string(la_fwd_workspace_bytes(a));
    run_case("la_fwd" + std::string(t.head_thr ? "_head_thr" : "") + ": " + name,
             [&]() -> int64_t { return t.head_thr ? la_fwd_head_thr(a, t.table, t.bs, t.hs, STREAM) : la_fwd(a, STREAM); }, kn, ws);
}
void fwd_case(const std::string& name, const la_fwd_args& a, const Knobs& kn = {}, const Thr& t = {}) { fwd_case(name, &a, kn, t); }

// the workspace a caller would give: the address WS with the bytes the library asks for
void give_workspace(la_fwd_args& a) {
    const int64_t need = la_fwd_workspace_bytes(&a);
    a.workspace = need > 0 ? fake<void>(WS) : nullptr;
    a.workspace_bytes = need > 0 ? static_cast<uint64_t>(need) : 0;
}
void contiguous(la_fwd_args& a, int64_t o_pad = 0) {
    const int64_t d = a.head_dim;
    a.q_head_stride = d; a.q_row_stride = d * a.num_heads; a.q_batch_stride = a.q_row_stride * a.seqlen_q;
    a.k_head_stride = d; a.k_row_stride = d * a.num_heads_k; a.k_batch_stride = a.k_row_stride * a.seqlen_k;
    a.v_head_stride = d; a.v_row_stride = d * a.num_heads_k; a.v_batch_stride = a.v_row_stride * a.seqlen_k;
    a.o_head_stride = d + o_pad; a.o_row_stride = a.o_head_stride * a.num_heads + o_pad; a.o_batch_stride = a.o_row_stride * a.seqlen_q + o_pad;
}
// a valid block: (batch 2, 300 queries, 500 keys, 4 heads on 2 K/V heads) unless given, every optional tensor present, the workspace given
la_fwd_args block(int dtype, int head_dim, bool lists, uint32_t flags = 0, int batch = 2, int sq = 300, int sk = 500, int h = 4, int hk = 2) {
    la_fwd_args a;
    memset(&a, 0, sizeof a);
    a.struct_size = sizeof a; a.dtype = dtype; a.flags = flags;
    a.q = fake<void>(Q); a.k = fake<void>(K); a.v = fake<void>(V); a.o = fake<void>(O); a.lse = fake<float>(LSE);
    a.batch = batch; a.seqlen_q = sq; a.seqlen_k = sk; a.num_heads = h; a.num_heads_k = hk; a.head_dim = a.head_dim_v = head_dim;
    contiguous(a);
    a.softmax_scale = 0.125f; a.thr = -3.0f;
    if (dtype == E4M3) {
        a.q_descale = fake<float>(QD); a.k_descale = fake<float>(KD); a.v_descale = fake<float>(VD);
        a.q_descale_batch_stride = a.k_descale_batch_stride = a.v_descale_batch_stride = hk;
        a.q_descale_head_stride = a.k_descale_head_stride = a.v_descale_head_stride = 1;
    }
    if (lists) { a.read_list = fake<int32_t>(RL); a.write_list = fake<int32_t>(WL); a.must_do_list = fake<int32_t>(MD); a.must_do_is_1d = 1; }
    int bm = 0, bn = 0;
    la_get_tile_sizes_ex(head_dim, dtype == E4M3 ? 1 : 2, flags, &bm, &bn);
    a.block_m = bm; a.block_n = bn;
    give_workspace(a);
    return a;
}
la_fwd_args varlen(la_fwd_args a) {
    a.cu_seqlens_q = fake<int32_t>(CUQ); a.cu_seqlens_k = fake<int32_t>(CUK); a.total_q = 517;
    give_workspace(a);
    return a;
}
template <class A, class M> A with(A a, M&& m) { m(a); return a; }
const char* dname(int dtype) { return dtype == BF16 ? "bf16" : dtype == FP16 ? "fp16" : dtype == E4M3 ? "e4m3" : "fp32"; }
std::string tag(int dtype, int d, bool lists) { return std::string(dname(dtype)) + " d" + std::to_string(d) + (lists ? " lists" : " dense"); }

// The longest dense key range of one launch (tests/golden/walk_bounds.json: the test holds these four to that file)
constexpr int kBoundBf16D256 = 102656, kBoundBf16D128 = 309760, kBoundE4m3D256 = 309760, kBoundE4m3D64 = 413376;

// ---- every `return` of fwd_run, in source order; each block is valid up to the check it names -----------------------------------------
void cases_fwd_returns() {
    const la_fwd_args b = block(BF16, 128, true), f = block(E4M3, 128, true), dn = block(BF16, 128, false);
    fwd_case("NULL block -> LA_ERR_NULL_ARG", nullptr);
    fwd_case("struct_size - 8 -> LA_ERR_STRUCT_SIZE", with(b, [](la_fwd_args& a) { a.struct_size -= 8; }));
    fwd_case("dtype fp32 -> LA_ERR_DTYPE", with(b, [](la_fwd_args& a) { a.dtype = FP32; }));
    fwd_case("dtype 7 -> LA_ERR_DTYPE", with(b, [](la_fwd_args& a) { a.dtype = 7; }));
    fwd_case("q NULL -> LA_ERR_NULL_ARG", with(b, [](la_fwd_args& a) { a.q = nullptr; }));
    fwd_case("o NULL -> LA_ERR_NULL_ARG", with(b, [](la_fwd_args& a) { a.o = nullptr; }));
    fwd_case("k NULL with keys -> LA_ERR_NULL_ARG", with(b, [](la_fwd_args& a) { a.k = nullptr; }));
    fwd_case("v NULL with keys -> LA_ERR_NULL_ARG", with(b, [](la_fwd_args& a) { a.v = nullptr; }));
    fwd_case("k and v NULL with seqlen_k == 0 -> the empty-keys fill", with(dn, [](la_fwd_args& a) { a.k = a.v = nullptr; a.seqlen_k = 0; }));
    const auto shape = [&](const char* what, void (*m)(la_fwd_args&)) { fwd_case(std::string(what) + " -> LA_ERR_SHAPE (sizes)", with(b, m)); };
    shape("batch 0", [](la_fwd_args& a) { a.batch = 0; });
    shape("seqlen_q 0", [](la_fwd_args& a) { a.seqlen_q = 0; });
    shape("seqlen_k -1", [](la_fwd_args& a) { a.seqlen_k = -1; });
    shape("num_heads 0", [](la_fwd_args& a) { a.num_heads = 0; });
    shape("num_heads_k 0", [](la_fwd_args& a) { a.num_heads_k = 0; });
    shape("head_dim 0", [](la_fwd_args& a) { a.head_dim = 0; });
    shape("head_dim_v -8", [](la_fwd_args& a) { a.head_dim_v = -8; });
    fwd_case("4 heads on 3 K/V heads -> LA_ERR_SHAPE (divisibility)", with(b, [](la_fwd_args& a) { a.num_heads_k = 3; }));
    fwd_case("bf16 head_dim 100 -> LA_ERR_HEAD_DIM (% 8)", with(b, [](la_fwd_args& a) { a.head_dim = a.head_dim_v = 100; }));
    fwd_case("e4m3 head_dim 72 -> LA_ERR_HEAD_DIM (% 16)", with(f, [](la_fwd_args& a) { a.head_dim = a.head_dim_v = 72; }));
    fwd_case("head_dim_v 64 != head_dim 128 -> LA_ERR_UNSUPPORTED", with(b, [](la_fwd_args& a) { a.head_dim_v = 64; }));
    fwd_case("reserved0 1 -> LA_ERR_UNSUPPORTED", with(b, [](la_fwd_args& a) { a.reserved0 = 1; }));
    fwd_case("flag 256 -> LA_ERR_UNSUPPORTED (unknown flag)", with(b, [](la_fwd_args& a) { a.flags |= 256u; }));
    fwd_case("LA_FLAG_LIST_INT16 without lists -> LA_ERR_UNSUPPORTED", with(dn, [](la_fwd_args& a) { a.flags |= LA_FLAG_LIST_INT16; }));
    fwd_case("bf16 head_dim 80 -> LA_ERR_HEAD_DIM (la_get_tile_sizes_ex)", with(b, [](la_fwd_args& a) { a.head_dim = a.head_dim_v = 80; }));
    fwd_case("e4m3 head_dim 80 -> LA_ERR_HEAD_DIM (la_get_tile_sizes_ex)", with(f, [](la_fwd_args& a) { a.head_dim = a.head_dim_v = 80; }));
    fwd_case("e4m3 LA_FLAG_KERNEL_128ROW -> LA_ERR_UNSUPPORTED (la_get_tile_sizes_ex)", with(f, [](la_fwd_args& a) { a.flags |= LA_FLAG_KERNEL_128ROW; }));
    fwd_case("block_m + 1 -> LA_ERR_TILE_MISMATCH", with(b, [](la_fwd_args& a) { a.block_m += 1; }));
    fwd_case("block_n 128 -> LA_ERR_TILE_MISMATCH", with(b, [](la_fwd_args& a) { a.block_n = 128; }));
    fwd_case("read list alone -> LA_ERR_LISTS", with(b, [](la_fwd_args& a) { a.write_list = nullptr; }));
    fwd_case("write list alone -> LA_ERR_LISTS", with(b, [](la_fwd_args& a) { a.read_list = nullptr; }));
    // the 12 strides: off the granularity (8 elements; 16 for the e4m3 q / k / v, whose o is bf16: + 8 passes there) and negative
    static int64_t la_fwd_args::* const strides[12] = {
        &la_fwd_args::q_batch_stride, &la_fwd_args::q_row_stride, &la_fwd_args::q_head_stride, &la_fwd_args::k_batch_stride,
        &la_fwd_args::k_row_stride,   &la_fwd_args::k_head_stride, &la_fwd_args::v_batch_stride, &la_fwd_args::v_row_stride,
        &la_fwd_args::v_head_stride,  &la_fwd_args::o_batch_stride, &la_fwd_args::o_row_stride,  &la_fwd_args::o_head_stride};
    static const char* const stride_names[12] = {"q_batch", "q_row", "q_head", "k_batch", "k_row", "k_head", "v_batch", "v_row", "v_head", "o_batch", "o_row", "o_head"};
    for (int i = 0; i < 12; ++i) {
        const std::string n = std::string(stride_names[i]) + "_stride";
        fwd_case("bf16 " + n + " + 4 -> LA_ERR_STRIDE (granularity 8)", with(b, [&](la_fwd_args& a) { a.*strides[i] += 4; }));
        fwd_case("bf16 " + n + " negative -> LA_ERR_STRIDE", with(b, [&](la_fwd_args& a) { a.*strides[i] = -(a.*strides[i]); }));
        fwd_case("e4m3 " + n + " + 8 -> " + (i < 9 ? "LA_ERR_STRIDE (granularity 16)" : "passes (o is bf16: granularity 8)"),
                 with(f, [&](la_fwd_args& a) { a.*strides[i] += 8; }));
        fwd_case("e4m3 " + n + " negative -> LA_ERR_STRIDE", with(f, [&](la_fwd_args& a) { a.*strides[i] = -(a.*strides[i]); }));
    }
    fwd_case("q_row_stride 0x40000000 -> LA_ERR_STRIDE (32-bit byte stride)", with(b, [](la_fwd_args& a) { a.q_row_stride = 0x40000000; }));
    fwd_case("o_row_stride 0x40000000 -> LA_ERR_STRIDE (32-bit byte stride)", with(b, [](la_fwd_args& a) { a.o_row_stride = 0x40000000; }));
    fwd_case("q_row_stride and o_row_stride 0x3ffffff8 -> passes", with(b, [](la_fwd_args& a) { a.q_row_stride = a.o_row_stride = 0x3ffffff8; }));
    fwd_case("bf16 k_row_stride 2^25 + 8 -> LA_ERR_STRIDE (LA_MAX_KV_ROW_STRIDE_BYTES)", with(b, [](la_fwd_args& a) { a.k_row_stride = (1 << 25) + 8; }));
    fwd_case("bf16 v_row_stride 2^25 + 8 -> LA_ERR_STRIDE (LA_MAX_KV_ROW_STRIDE_BYTES)", with(b, [](la_fwd_args& a) { a.v_row_stride = (1 << 25) + 8; }));
    fwd_case("bf16 k_row_stride and v_row_stride 2^25 -> passes", with(b, [](la_fwd_args& a) { a.k_row_stride = a.v_row_stride = 1 << 25; }));
    fwd_case("e4m3 k_row_stride 2^26 + 16 -> LA_ERR_STRIDE (LA_MAX_KV_ROW_STRIDE_BYTES)", with(f, [](la_fwd_args& a) { a.k_row_stride = (1 << 26) + 16; }));
    fwd_case("e4m3 v_row_stride 2^26 + 16 -> LA_ERR_STRIDE (LA_MAX_KV_ROW_STRIDE_BYTES)", with(f, [](la_fwd_args& a) { a.v_row_stride = (1 << 26) + 16; }));
    fwd_case("e4m3 k_row_stride and v_row_stride 2^26 -> passes", with(f, [](la_fwd_args& a) { a.k_row_stride = a.v_row_stride = 1 << 26; }));
    fwd_case("q + 8 bytes -> LA_ERR_STRIDE (base)", with(b, [](la_fwd_args& a) { a.q = fake<void>(Q + 8); }));
    fwd_case("k + 8 bytes -> LA_ERR_STRIDE (base)", with(b, [](la_fwd_args& a) { a.k = fake<void>(K + 8); }));
    fwd_case("v + 8 bytes -> LA_ERR_STRIDE (base)", with(b, [](la_fwd_args& a) { a.v = fake<void>(V + 8); }));
    fwd_case("o + 8 bytes -> LA_ERR_STRIDE (base)", with(b, [](la_fwd_args& a) { a.o = fake<void>(O + 8); }));
    // the varlen checks
    fwd_case("cu_seqlens_q alone -> LA_ERR_NULL_ARG", with(varlen(b), [](la_fwd_args& a) { a.cu_seqlens_k = nullptr; }));
    fwd_case("cu_seqlens_k alone -> LA_ERR_NULL_ARG", with(varlen(b), [](la_fwd_args& a) { a.cu_seqlens_q = nullptr; }));
    fwd_case("varlen lists under LA_FLAG_KERNEL_128ROW -> LA_ERR_UNSUPPORTED", varlen(block(BF16, 128, true, LA_FLAG_KERNEL_128ROW)));
    fwd_case("varlen lists at bf16 head_dim 256 -> LA_ERR_UNSUPPORTED", varlen(block(BF16, 256, true)));
    fwd_case("varlen total_q -1 -> LA_ERR_SHAPE", with(varlen(b), [](la_fwd_args& a) { a.total_q = -1; }));
    fwd_case("varlen with a q-tile window -> LA_ERR_SHAPE", with(varlen(b), [](la_fwd_args& a) { a.q_tile_count = 1; }));
    // the e4m3 workspace (checked before the int16 row and the window)
    fwd_case("e4m3 workspace NULL -> LA_ERR_WORKSPACE", with(f, [](la_fwd_args& a) { a.workspace = nullptr; }));
    fwd_case("e4m3 workspace one byte short -> LA_ERR_WORKSPACE", with(f, [](la_fwd_args& a) { a.workspace_bytes -= 1; }));
    fwd_case("e4m3 workspace + 8 bytes -> LA_ERR_WORKSPACE (alignment)", with(f, [](la_fwd_args& a) { a.workspace = fake<void>(WS + 8); }));
    fwd_case("e4m3 workspace missing wins over an int16 row too long -> LA_ERR_WORKSPACE",
             with(block(E4M3, 128, true, LA_FLAG_LIST_INT16, 1, 300, 32767 * 64, 2, 1), [](la_fwd_args& a) { a.workspace = nullptr; }));
    // LA_FLAG_LIST_INT16: a row of k_tiles + 1 entries above 32767
    fwd_case("bf16 int16 lists, 32767 key tiles -> LA_ERR_SEQLEN (row too long)", block(BF16, 128, true, LA_FLAG_LIST_INT16, 1, 300, 32767 * 64, 2, 1));
    fwd_case("e4m3 int16 lists, 32767 key tiles -> LA_ERR_SEQLEN (row too long)", block(E4M3, 128, true, LA_FLAG_LIST_INT16, 1, 300, 32767 * 64, 2, 1));
    // every LA_ERR_Q_WINDOW (300 queries: 2 q-tiles of 256 rows; under LA_FLAG_HALF_VOTE 3 list rows of 128)
    fwd_case("q_tile_count 0 with q_tile_begin 1 -> LA_ERR_Q_WINDOW", with(b, [](la_fwd_args& a) { a.q_tile_begin = 1; }));
    fwd_case("q_tile_begin -1 -> LA_ERR_Q_WINDOW", with(b, [](la_fwd_args& a) { a.q_tile_begin = -1; a.q_tile_count = 1; }));
    fwd_case("q_tile_count -1 -> LA_ERR_Q_WINDOW", with(b, [](la_fwd_args& a) { a.q_tile_count = -1; }));
    fwd_case("window [1, 3) of 2 q-tiles -> LA_ERR_Q_WINDOW", with(b, [](la_fwd_args& a) { a.q_tile_begin = 1; a.q_tile_count = 2; }));
    const la_fwd_args hv = block(BF16, 128, true, LA_FLAG_HALF_VOTE);
    fwd_case("half-vote window on an odd q-tile -> LA_ERR_Q_WINDOW", with(hv, [](la_fwd_args& a) { a.q_tile_begin = 1; a.q_tile_count = 2; }));
    fwd_case("half-vote window of an odd count short of the last -> LA_ERR_Q_WINDOW", with(hv, [](la_fwd_args& a) { a.q_tile_begin = 0; a.q_tile_count = 1; }));
    fwd_case("half-vote window of an odd count that reaches the last -> passes", with(hv, [](la_fwd_args& a) { a.q_tile_begin = 2; a.q_tile_count = 1; }));
    fwd_case("half-vote window past the end -> LA_ERR_Q_WINDOW (range check first)", with(hv, [](la_fwd_args& a) { a.q_tile_begin = 2; a.q_tile_count = 2; }));
    // the 128-row template's LDS bound, on both sides of the limit (the stand-in answers what the case sets)
    const la_fwd_args r128 = block(BF16, 128, true, LA_FLAG_KERNEL_128ROW);
    Knobs over; over.lds_v2 = 160 * 1024 + 1;
    Knobs at; at.lds_v2 = 160 * 1024;
    fwd_case("128-row template one byte over the LDS limit -> LA_ERR_SEQLEN", r128, over);
    fwd_case("128-row template at the LDS limit -> passes", r128, at);
    fwd_case("128-row template, 30000 key tiles by the restated arithmetic -> LA_ERR_SEQLEN", block(BF16, 128, true, LA_FLAG_KERNEL_128ROW, 1, 300, 30000 * 64, 2, 1));
    // batch * heads * q_tiles above 2^31 - 1
    fwd_case("bf16 65536 x 32768 items -> LA_ERR_SHAPE (item count)", block(BF16, 128, true, 0, 65536, 256, 500, 32768, 2));
    fwd_case("e4m3 65536 x 32768 items -> LA_ERR_SHAPE (item count)", block(E4M3, 128, true, 0, 65536, 256, 500, 32768, 2));
    fwd_case("bf16 65536 x 32767 items -> passes", block(BF16, 128, true, 0, 65536, 256, 500, 32767, 1));
}

// ---- table_status of la_fwd_head_thr: three outcomes (no table / LA_ERR_LISTS on a dense launch / LA_ERR_STRIDE) on five call sites ---
// The two split sites are dense by construction, so a table there is always LA_ERR_LISTS; LA_ERR_STRIDE and a table that passes need lists.
void cases_table_status() {
    const Thr none{nullptr, -1, -1, true}, good = table(), neg_bs = table(THR, -1, 1), neg_hs = table(THR, 4, -1), off4 = table(THR + 2);
    const auto site = [&](const std::string& where, const la_fwd_args& a, bool dense) {
        fwd_case(where + ", thr_head NULL (strides not looked at) -> la_fwd", a, {}, none);
        fwd_case(where + ", table" + (dense ? " on a dense launch -> LA_ERR_LISTS" : " -> passes, in FwdParams"), a, {}, good);
        fwd_case(where + ", table with a negative batch stride -> " + (dense ? "LA_ERR_LISTS first" : "LA_ERR_STRIDE"), a, {}, neg_bs);
        if (!dense) {
            fwd_case(where + ", table with a negative head stride -> LA_ERR_STRIDE", a, {}, neg_hs);
            fwd_case(where + ", table off a 4-byte boundary -> LA_ERR_STRIDE", a, {}, off4);
        }
    };
    site("empty keys, lists", block(BF16, 128, true, 0, 2, 300, 0), false);
    site("empty keys, dense", block(BF16, 128, false, 0, 2, 300, 0), true);
    site("e4m3 split", block(E4M3, 64, false, 0, 2, 131, kBoundE4m3D64 + 1), true);
    site("e4m3 one launch, lists", block(E4M3, 128, true), false);
    site("e4m3 one launch, dense", block(E4M3, 128, false), true);
    site("bf16 split", block(BF16, 256, false, 0, 2, 131, kBoundBf16D256 + 1), true);
    site("bf16 one launch, lists", block(BF16, 128, true), false);
    site("bf16 one launch, dense", block(BF16, 128, false), true);
    site("128-row template, lists", block(BF16, 128, true, LA_FLAG_KERNEL_128ROW), false);
    // a failing table comes after the LAST of la_fwd's own checks of its path
    fwd_case("bad table and a bad window -> LA_ERR_Q_WINDOW", with(block(BF16, 128, true), [](la_fwd_args& a) { a.q_tile_begin = 1; }), {}, neg_bs);
    fwd_case("bad table and too many items -> LA_ERR_SHAPE", block(BF16, 128, true, 0, 65536, 256, 500, 32768, 2), {}, neg_bs);
    fwd_case("bad table and no e4m3 workspace -> LA_ERR_WORKSPACE", with(block(E4M3, 128, true), [](la_fwd_args& a) { a.workspace = nullptr; }), {}, neg_bs);
    fwd_case("table and lists too long for one launch (bf16) -> LA_ERR_SEQLEN", block(BF16, 256, true, 0, 2, 131, kBoundBf16D256 + 1), {}, good);
    fwd_case("table and lists too long for one launch (e4m3) -> LA_ERR_SEQLEN", block(E4M3, 64, true, 0, 2, 131, kBoundE4m3D64 + 1), {}, good);
    fwd_case("table on a bf16 split without its workspace -> LA_ERR_SEQLEN", with(block(BF16, 256, false, 0, 2, 131, kBoundBf16D256 + 1), [](la_fwd_args& a) { a.workspace = nullptr; }), {}, good);
    Knobs over; over.lds_v2 = 160 * 1024 + 1;
    fwd_case("bad table and the 128-row template over its LDS limit -> LA_ERR_SEQLEN", block(BF16, 128, true, LA_FLAG_KERNEL_128ROW), over, neg_bs);
}

// ---- launch shapes: what one launch is handed -------------------------------------------------------------------------------------------
void cases_launch_shapes() {
    static const int dims[] = {64, 96, 128, 192, 256};
    struct Form { int dtype; uint32_t flags; const char* name; };
    static const Form forms[] = {{BF16, 0, "bf16"}, {FP16, 0, "fp16"}, {E4M3, 0, "e4m3 P as the reference"}, {E4M3, LA_FLAG_FP8_MFMA_ROWSUM, "e4m3 matrix-pipe row sums"},
                                 {E4M3, LA_FLAG_FP8_ENCODED_P, "e4m3 encoded P"}, {E4M3, LA_FLAG_FP8_ENCODED_P | LA_FLAG_FP8_MFMA_ROWSUM, "e4m3 both P flags (encoded wins)"}};
    for (const Form& fm : forms)
        for (int d : dims)
            for (int lists = 0; lists < 2; ++lists) {
                const std::string n = std::string(fm.name) + " d" + std::to_string(d) + (lists ? " lists" : " dense");
                const la_fwd_args a = block(fm.dtype, d, lists != 0, fm.flags);
                fwd_case(n + ", workspace -> one launch, ticket counters", a);
                if (fm.dtype != E4M3) {
                    fwd_case(n + ", no workspace -> one launch, static map", with(a, [](la_fwd_args& x) { x.workspace = nullptr; x.workspace_bytes = 0; }));
                    fwd_case(n + ", LA_FLAG_STATIC_SCHED with a workspace -> static map", with(a, [](la_fwd_args& x) { x.flags |= LA_FLAG_STATIC_SCHED; }));
                } else if (fm.flags == 0) {
                    fwd_case(n + ", LA_FLAG_STATIC_SCHED -> no work_counter", with(a, [](la_fwd_args& x) { x.flags |= LA_FLAG_STATIC_SCHED; }));
                    fwd_case(n + ", LA_FLAG_V_PREPARED -> no prepare pass", with(a, [](la_fwd_args& x) { x.flags |= LA_FLAG_V_PREPARED; }));
                }
            }
    // the optional 16-bit workspace is used only when it is whole and aligned
    const la_fwd_args b = block(BF16, 128, true);
    fwd_case("bf16 workspace of 1023 bytes -> static map", with(b, [](la_fwd_args& a) { a.workspace_bytes = 1023; }));
    fwd_case("bf16 workspace + 8 bytes -> static map", with(b, [](la_fwd_args& a) { a.workspace = fake<void>(WS + 8); }));
    // LA_FLAG_KERNEL_128ROW: the template at 64 / 128 / 256 (q-tile 128 at 64 and 128), LA_ERR_HEAD_DIM at 96 / 192
    for (int dtype : {BF16, FP16})
        for (int d : dims)
            for (int lists = 0; lists < 2; ++lists) {
                const bool has = d != 96 && d != 192;
                const la_fwd_args a = block(dtype, d, lists != 0, LA_FLAG_KERNEL_128ROW);
                fwd_case(tag(dtype, d, lists) + " LA_FLAG_KERNEL_128ROW -> " + (has ? "launch_fwd_bf16_v2" : "LA_ERR_HEAD_DIM"), a);
                if (has && dtype == BF16) fwd_case(tag(dtype, d, lists) + " LA_FLAG_KERNEL_128ROW, no workspace", with(a, [](la_fwd_args& x) { x.workspace = nullptr; x.workspace_bytes = 0; }));
            }
    fwd_case("bf16 d128 dense LA_FLAG_KERNEL_128ROW with a workspace given anyway -> no work_counter", with(block(BF16, 128, false, LA_FLAG_KERNEL_128ROW), [](la_fwd_args& a) { a.workspace = fake<void>(WS); a.workspace_bytes = 1024; }));
    // LA_FLAG_HALF_VOTE: 300 queries are 3 list rows of 128 (odd) and 2 items of 256
    for (int d : {64, 96, 128, 192, 256})
        for (int lists = 0; lists < 2; ++lists) {
            const la_fwd_args a = block(BF16, d, lists != 0, LA_FLAG_HALF_VOTE);
            fwd_case(tag(BF16, d, lists) + " LA_FLAG_HALF_VOTE, full launch" + (d > 128 ? " (no effect at this head dim)" : ""), a);
        }
    const la_fwd_args hv = block(FP16, 128, true, LA_FLAG_HALF_VOTE);
    fwd_case("fp16 d128 lists LA_FLAG_HALF_VOTE window [0, 2) -> item 0", with(hv, [](la_fwd_args& a) { a.q_tile_count = 2; }));
    fwd_case("fp16 d128 lists LA_FLAG_HALF_VOTE window [2, 3) -> item 1", with(hv, [](la_fwd_args& a) { a.q_tile_begin = 2; a.q_tile_count = 1; }));
    fwd_case("fp16 d128 lists LA_FLAG_HALF_VOTE window [0, 3) -> both items", with(hv, [](la_fwd_args& a) { a.q_tile_count = 3; }));
    fwd_case("bf16 d128 lists LA_FLAG_HALF_VOTE | LA_FLAG_KERNEL_128ROW -> the template wins", block(BF16, 128, true, LA_FLAG_HALF_VOTE | LA_FLAG_KERNEL_128ROW));
    fwd_case("e4m3 d128 lists LA_FLAG_HALF_VOTE -> no effect", block(E4M3, 128, true, LA_FLAG_HALF_VOTE));
    fwd_case("bf16 d128 lists LA_FLAG_HALF_VOTE, 1300 queries, window [4, 8)", with(block(BF16, 128, true, LA_FLAG_HALF_VOTE, 2, 1300), [](la_fwd_args& a) { a.q_tile_begin = 4; a.q_tile_count = 4; }));
    // q-tile windows without the flag
    fwd_case("bf16 d128 lists window [1, 2)", with(b, [](la_fwd_args& a) { a.q_tile_begin = 1; a.q_tile_count = 1; }));
    fwd_case("bf16 d256 dense window [1, 3) of 3", with(block(BF16, 256, false), [](la_fwd_args& a) { a.q_tile_begin = 1; a.q_tile_count = 2; }));
    fwd_case("e4m3 d128 lists window [0, 1) under LA_FLAG_V_PREPARED", with(block(E4M3, 128, true, LA_FLAG_V_PREPARED), [](la_fwd_args& a) { a.q_tile_count = 1; }));
    // scalars
    for (int dtype : {BF16, E4M3}) {
        fwd_case(tag(dtype, 128, true) + " LA_FLAG_EXACT_RESCALE -> rescale_tau 0", block(dtype, 128, true, LA_FLAG_EXACT_RESCALE));
        fwd_case(tag(dtype, 128, true) + " softmax_scale 0 -> scale_log2 2^-100", with(block(dtype, 128, true), [](la_fwd_args& a) { a.softmax_scale = 0.0f; }));
        fwd_case(tag(dtype, 128, true) + " LA_FLAG_LIST_INT16 -> list_int16 1", block(dtype, 128, true, LA_FLAG_LIST_INT16));
        fwd_case(tag(dtype, 128, true) + " 4-D must_do_list, no lse", with(block(dtype, 128, true), [](la_fwd_args& a) { a.must_do_is_1d = 0; a.lse = nullptr; }));
        fwd_case(tag(dtype, 128, false) + " MHA 4 on 4", block(dtype, 128, false, 0, 2, 300, 500, 4, 4));
        fwd_case(tag(dtype, 128, true) + " MQA 4 on 1", block(dtype, 128, true, 0, 2, 300, 500, 4, 1));
        fwd_case(tag(dtype, 128, false) + " batch 1, 1 query, 1 key", block(dtype, 128, false, 0, 1, 1, 1, 1, 1));
        fwd_case(tag(dtype, 128, false) + " padded strides", with(block(dtype, 128, false), [](la_fwd_args& a) { contiguous(a, 64); a.k_row_stride += 256; a.v_batch_stride += 1024; a.q_head_stride += 16; }));
    }
    // varlen
    for (const Form& fm : {forms[0], forms[1], forms[2]})
        for (int d : {64, 128, 256})
            for (int lists = 0; lists < 2; ++lists) {
                const bool refused = lists && d > 128 && fm.dtype != E4M3;
                fwd_case(std::string("varlen ") + tag(fm.dtype, d, lists) + (refused ? " -> LA_ERR_UNSUPPORTED" : " -> one launch"), varlen(block(fm.dtype, d, lists != 0)));
            }
    fwd_case("varlen bf16 d128 dense LA_FLAG_KERNEL_128ROW", varlen(block(BF16, 128, false, LA_FLAG_KERNEL_128ROW)));
    fwd_case("varlen e4m3 d128 dense LA_FLAG_V_PREPARED -> no prepare pass", varlen(block(E4M3, 128, false, LA_FLAG_V_PREPARED)));
    // no keys: o = 0, lse = +inf (varlen: rows are total_q, the LSE by a 32-bit fill)
    Knobs f0; f0.fail_at = 0; f0.fail_err = hipErrorInvalidConfiguration;
    Knobs f1; f1.fail_at = 1; f1.fail_err = hipErrorInvalidDevicePointer;
    for (int dtype : {BF16, E4M3}) {
        const la_fwd_args e = block(dtype, 128, false, 0, 2, 300, 0);
        fwd_case(tag(dtype, 128, false) + " seqlen_k 0 -> launch_empty_k_fill", e);
        fwd_case(tag(dtype, 128, false) + " seqlen_k 0, the fill fails -> LA_ERR_LAUNCH", e, f0);
        fwd_case(tag(dtype, 128, false) + " varlen seqlen_k 0 -> fill of total_q rows + hipMemsetD32Async", varlen(e));
        fwd_case(tag(dtype, 128, false) + " varlen seqlen_k 0, the fill fails -> no hipMemsetD32Async", varlen(e), f0);
        fwd_case(tag(dtype, 128, false) + " varlen seqlen_k 0, hipMemsetD32Async fails -> LA_ERR_LAUNCH", varlen(e), f1);
        fwd_case(tag(dtype, 128, false) + " varlen seqlen_k 0, no lse -> the fill alone", with(varlen(e), [](la_fwd_args& a) { a.lse = nullptr; }));
        fwd_case(tag(dtype, 128, false) + " varlen seqlen_k 0, total_q 0 -> the fill alone", with(varlen(e), [](la_fwd_args& a) { a.total_q = 0; }));
        fwd_case(tag(dtype, 128, true) + " seqlen_k 0 with lists -> the fill (the lists are left alone)", block(dtype, 128, true, 0, 2, 300, 0));
    }
    fwd_case("e4m3 d128 dense seqlen_k 0 without a workspace -> the fill (checked behind it)", with(block(E4M3, 128, false, 0, 2, 300, 0), [](la_fwd_args& a) { a.workspace = nullptr; a.workspace_bytes = 0; }));
    // a launcher error on the one-launch paths
    fwd_case("bf16 d128 lists, the launch fails -> LA_ERR_LAUNCH", b, f0);
    fwd_case("bf16 d128 lists LA_FLAG_KERNEL_128ROW, the launch fails -> LA_ERR_LAUNCH", block(BF16, 128, true, LA_FLAG_KERNEL_128ROW), f0);
    fwd_case("e4m3 d128 lists, the prepare pass fails -> no forward", block(E4M3, 128, true), f0);
    fwd_case("e4m3 d128 lists, the forward fails -> LA_ERR_LAUNCH", block(E4M3, 128, true), f1);
}

// ---- the split of a long dense key range into runs ----------------------------------------------------------------------------------
void cases_split() {
    struct Path { int dtype, d, bound, calls_per_run; };
    static const Path paths[] = {{BF16, 256, kBoundBf16D256, 1}, {BF16, 128, kBoundBf16D128, 1}, {FP16, 256, kBoundBf16D256, 1},
                                 {E4M3, 256, kBoundE4m3D256, 2}, {E4M3, 64, kBoundE4m3D64, 2}};
    for (const Path& p : paths) {
        const std::string n = tag(p.dtype, p.d, false);
        const auto blk = [&](int sk, bool lists = false, uint32_t flags = 0) {
            la_fwd_args a = block(p.dtype, p.d, lists, flags, 2, 131, sk, 4, 2);
            contiguous(a, 64);                                           // padded O strides: the combine gets the caller's, the runs contiguous ones
            return a;
        };
        if (p.dtype == FP16) {                                           // fp16 shares the bf16 path: the f16 flag of the runs and the merge
            fwd_case(n + " bound + 1 keys -> 2 runs + combine (f16)", blk(p.bound + 1));
            continue;
        }
        fwd_case(n + " the bound -> one launch", blk(p.bound));
        fwd_case(n + " bound + 1 keys -> 2 runs + combine", blk(p.bound + 1));
        fwd_case(n + " twice the bound + 1 keys -> 3 runs + combine", blk(2 * p.bound + 1));
        fwd_case(n + " bound + 64 + 37 keys -> 2 runs, a ragged last tile", blk(p.bound + 64 + 37));
        fwd_case(n + " bound + 1 keys, no lse, LA_FLAG_STATIC_SCHED -> runs without a work_counter", with(blk(p.bound + 1, false, LA_FLAG_STATIC_SCHED), [](la_fwd_args& a) { a.lse = nullptr; }));
        const la_fwd_args s = blk(p.bound + 1);
        // the refusals
        fwd_case(n + " bound + 1 keys with lists -> LA_ERR_SEQLEN (lists keep the bound)", blk(p.bound + 1, true));
        if (p.dtype == E4M3 || p.d <= 128) fwd_case(n + " bound + 1 keys, varlen with lists -> LA_ERR_SEQLEN", varlen(blk(p.bound + 1, true)));
        fwd_case(n + " bound + 1 keys, varlen -> LA_ERR_SEQLEN", varlen(s));
        fwd_case(n + " bound + 1 keys, varlen with a workspace of 2^40 bytes -> LA_ERR_SEQLEN", with(varlen(s), [](la_fwd_args& a) { a.workspace_bytes = 1ull << 40; }));
        // (131 queries are one q-tile of 256 rows: the window needs a problem of several)
        fwd_case(n + " bound + 1 keys, 600 queries, the window [0, 1) -> LA_ERR_SEQLEN", with(block(p.dtype, p.d, false, 0, 2, 600, p.bound + 1, 4, 2), [](la_fwd_args& a) { a.q_tile_count = 1; }));
        fwd_case(n + " bound + 1 keys, 131 queries, the window [0, all) -> splits", with(s, [&](la_fwd_args& a) { a.q_tile_count = (131 + a.block_m - 1) / a.block_m; }));
        if (p.dtype == E4M3) fwd_case(n + " bound + 1 keys, LA_FLAG_V_PREPARED -> LA_ERR_SEQLEN", with(s, [](la_fwd_args& a) { a.flags |= LA_FLAG_V_PREPARED; }));
        else fwd_case(n + " bound + 1 keys, LA_FLAG_V_PREPARED -> splits (the flag means nothing to bf16 / fp16)", with(s, [](la_fwd_args& a) { a.flags |= LA_FLAG_V_PREPARED; }));
        fwd_case(n + " bound + 1 keys, no workspace -> " + (p.dtype == E4M3 ? "LA_ERR_WORKSPACE" : "LA_ERR_SEQLEN"), with(s, [](la_fwd_args& a) { a.workspace = nullptr; }));
        fwd_case(n + " bound + 1 keys, workspace one byte short -> " + (p.dtype == E4M3 ? "LA_ERR_WORKSPACE" : "LA_ERR_SEQLEN"), with(s, [](la_fwd_args& a) { a.workspace_bytes -= 1; }));
        fwd_case(n + " bound + 1 keys, workspace + 8 bytes -> " + (p.dtype == E4M3 ? "LA_ERR_WORKSPACE" : "LA_ERR_SEQLEN"), with(s, [](la_fwd_args& a) { a.workspace = fake<void>(WS + 8); }));
        fwd_case(n + " bound + 1 keys, a workspace of the ticket counters alone -> " + (p.dtype == E4M3 ? "LA_ERR_WORKSPACE" : "LA_ERR_SEQLEN"), with(s, [](la_fwd_args& a) { a.workspace_bytes = 1024; }));
        // a launcher error: what was and was not launched after it
        Knobs k;
        k.fail_err = hipErrorLaunchFailure;
        for (int at = 0; at <= 2 * p.calls_per_run; ++at) {
            k.fail_at = at;
            fwd_case(n + " bound + 1 keys, launcher call " + std::to_string(at) + " fails (" + (at == 2 * p.calls_per_run ? "the combine" : "run " + std::to_string(at / p.calls_per_run)) + ") -> LA_ERR_LAUNCH", s, k);
        }
    }
    // the other head dims split too: one case each at its own bound + 1 (bounds of tests/golden/walk_bounds.json)
    fwd_case("bf16 d64 dense 413377 keys -> 2 runs", block(BF16, 64, false, 0, 1, 131, 413376 + 1, 2, 1));
    fwd_case("bf16 d96 dense 309761 keys -> 2 runs", block(BF16, 96, false, 0, 1, 131, 309760 + 1, 2, 1));
    fwd_case("bf16 d192 dense 102657 keys -> 2 runs", block(BF16, 192, false, 0, 1, 131, 102656 + 1, 2, 1));
    fwd_case("e4m3 d96 dense 413377 keys -> 2 runs", block(E4M3, 96, false, 0, 1, 131, 413376 + 1, 2, 1));
    fwd_case("e4m3 d128 dense 413377 keys -> 2 runs", block(E4M3, 128, false, 0, 1, 131, 413376 + 1, 2, 1));
    fwd_case("e4m3 d192 dense 309761 keys -> 2 runs", block(E4M3, 192, false, 0, 1, 131, 309760 + 1, 2, 1));
    // half-vote lists have a larger walk: the bound of a listed launch moves with the flag (dense launches ignore it)
    fwd_case("bf16 d128 dense LA_FLAG_HALF_VOTE at the bound -> one launch", block(BF16, 128, false, LA_FLAG_HALF_VOTE, 1, 131, kBoundBf16D128, 2, 1));
    fwd_case("bf16 d128 lists LA_FLAG_HALF_VOTE at the bound of the plain walk", block(BF16, 128, true, LA_FLAG_HALF_VOTE, 1, 131, kBoundBf16D128, 2, 1));
    // LA_FLAG_KERNEL_128ROW never splits
    fwd_case("bf16 d256 dense LA_FLAG_KERNEL_128ROW bound + 1 keys -> the template's own bound", block(BF16, 256, false, LA_FLAG_KERNEL_128ROW, 1, 131, kBoundBf16D256 + 1, 2, 1));
}

// ---- la_fwd_workspace_bytes on a grid ---------------------------------------------------------------------------------------------------
void grid_workspace_bytes() {
    static const int lens[] = {0, 1, 500, 102656, 102657, 205313, 309760, 309761, 619521, 413376, 413377, 826753};
    printf("\"workspace_grid_seqlen_k\":[");
    for (size_t i = 0; i < sizeof lens / sizeof *lens; ++i) printf("%s%d", i ? "," : "", lens[i]);
    printf("],\n\"workspace_grid\":{");
    bool first = true;
    const auto row = [&](const std::string& name, la_fwd_args a) {
        printf("%s\n\"%s\":[", first ? "" : ",", name.c_str());
        first = false;
        for (size_t i = 0; i < sizeof lens / sizeof *lens; ++i) {
            a.seqlen_k = lens[i];
            printf("%s%lld", i ? "," : "", static_cast<long long>(la_fwd_workspace_bytes(&a)));
        }
        printf("]");
    };
    for (int dtype : {BF16, FP16, E4M3, FP32})
        for (int d : {64, 80, 96, 128, 192, 256})                        // 80: not instantiated
            for (int lists = 0; lists < 2; ++lists)
                for (uint32_t flags : {0u, LA_FLAG_STATIC_SCHED, LA_FLAG_KERNEL_128ROW})
                    for (int vl = 0; vl < 2; ++vl) {
                        la_fwd_args a = block(dtype, d, lists != 0, flags, 2, 131, 500, 4, 2);
                        if (vl) a = varlen(a);
                        row(tag(dtype, d, lists) + " flags " + std::to_string(flags) + (vl ? " varlen" : " fixed"), a);
                    }
    // blocks the bf16 / fp16 arm answers without checking, and the codes of the e4m3 arm for the same blocks
    for (int dtype : {BF16, E4M3}) {
        const la_fwd_args a = block(dtype, 256, false, 0, 2, 131, 500, 4, 2);
        const std::string n = std::string(dname(dtype)) + " d256 dense, ";
        row(n + "num_heads_k 0", with(a, [](la_fwd_args& x) { x.num_heads_k = 0; }));
        row(n + "num_heads 0", with(a, [](la_fwd_args& x) { x.num_heads = 0; }));
        row(n + "batch 0", with(a, [](la_fwd_args& x) { x.batch = 0; }));
        row(n + "seqlen_q 0", with(a, [](la_fwd_args& x) { x.seqlen_q = 0; }));
        row(n + "head_dim_v 0", with(a, [](la_fwd_args& x) { x.head_dim_v = 0; }));
        row(n + "head_dim_v 64", with(a, [](la_fwd_args& x) { x.head_dim_v = 64; }));
        row(n + "head_dim_v 100 (partial O rounded up to 16 bytes)", with(a, [](la_fwd_args& x) { x.head_dim_v = 100; x.batch = 1; x.seqlen_q = 1; x.num_heads = 1; }));
        row(n + "unknown flag 256", with(a, [](la_fwd_args& x) { x.flags = 256u; }));
        row(n + "LA_FLAG_V_PREPARED", with(a, [](la_fwd_args& x) { x.flags = LA_FLAG_V_PREPARED; }));
        row(n + "LA_FLAG_HALF_VOTE | LA_FLAG_STATIC_SCHED", with(a, [](la_fwd_args& x) { x.flags = LA_FLAG_HALF_VOTE | LA_FLAG_STATIC_SCHED; }));
        row(n + "cu_seqlens_k alone", with(a, [](la_fwd_args& x) { x.cu_seqlens_k = fake<int32_t>(CUK); }));
        row(n + "struct_size 0", with(a, [](la_fwd_args& x) { x.struct_size = 0; }));
    }
    {
        la_fwd_args a = block(BF16, 256, false, 0, 2, 131, -5, 4, 2);
        printf(",\n\"bf16 seqlen_k -5\":[%lld]", static_cast<long long>(la_fwd_workspace_bytes(&a)));
        a.dtype = E4M3;
        printf(",\n\"e4m3 seqlen_k -5\":[%lld]", static_cast<long long>(la_fwd_workspace_bytes(&a)));
        printf(",\n\"NULL block\":[%lld]", static_cast<long long>(la_fwd_workspace_bytes(nullptr)));
    }
    printf("},\n");
}

// ---- every other entry point: one good case and one case per early return ---------------------------------------------------------------
template <class A, class Fn, class M>
void args_case(const std::string& name, const A& base, Fn fn, M&& m, const Knobs& kn = {}) {
    A a = base;
    m(a);
    run_case(name, [&]() -> int64_t { return fn(&a, STREAM); }, kn);
}
const auto keep = [](auto&) {};

template <class A> A prep_base() {              // what la_qk_prep_args, la_qk_prep_fp8_args and la_qk_prep_smooth_args share
    A a;
    memset(&a, 0, sizeof a);
    a.struct_size = sizeof a; a.in_dtype = BF16; a.norm_mode = LA_NORM_TOKEN;
    a.x = fake<void>(X); a.out = fake<void>(OUT);
    a.batch = 2; a.seqlen = 100; a.num_heads = 4; a.head_dim = 128;
    a.x_head_stride = a.out_head_stride = 128; a.x_row_stride = a.out_row_stride = 512; a.x_batch_stride = a.out_batch_stride = 51200;
    a.weight = fake<float>(0x50000000); a.eps = 1e-6f; a.pos_offset = 0;
    for (int i = 0; i < 3; ++i) a.rope_table[i] = fake<float>(0x51000000 + 0x1000000 * i);
    a.axis_extent[0] = 5; a.axis_extent[1] = 5; a.axis_extent[2] = 4;
    a.axis_pairs[0] = 16; a.axis_pairs[1] = 24; a.axis_pairs[2] = 24;
    return a;
}
template <class A> void scale_fields(A& a) {
    a.heads_per_scale = 2;
    a.descale = fake<float>(0x54000000); a.descale_batch_stride = 2; a.descale_head_stride = 1;
    a.amax = fake<float>(0x55000000); a.amax_batch_stride = 2; a.amax_head_stride = 1;
}
// the returns of qk_prep_check_and_fill, reached through entry point `fn` with the base block `b`
template <class A, class Fn>
void cases_prep_shared(const std::string& e, const A& b, Fn fn) {
    args_case(e + ": norm_mode 3 -> LA_ERR_UNSUPPORTED", b, fn, [](A& a) { a.norm_mode = 3; });
    args_case(e + ": seqlen 0 -> LA_ERR_SHAPE", b, fn, [](A& a) { a.seqlen = 0; });
    args_case(e + ": batch 0 -> LA_ERR_SHAPE", b, fn, [](A& a) { a.batch = 0; });
    args_case(e + ": head_dim 0 -> LA_ERR_SHAPE", b, fn, [](A& a) { a.head_dim = 0; });
    args_case(e + ": head_dim 100 -> LA_ERR_HEAD_DIM", b, fn, [](A& a) { a.head_dim = 100; });
    args_case(e + ": head_dim 264 -> LA_ERR_HEAD_DIM", b, fn, [](A& a) { a.head_dim = 264; });
    args_case(e + ": LA_NORM_TOKEN with 130 x 128 elements -> LA_ERR_UNSUPPORTED", b, fn, [](A& a) { a.num_heads = 130; });
    args_case(e + ": LA_NORM_HEAD with 130 x 128 elements -> passes", b, fn, [](A& a) { a.num_heads = 130; a.norm_mode = LA_NORM_HEAD; });
    args_case(e + ": x + 8 bytes -> LA_ERR_STRIDE", b, fn, [](A& a) { a.x = fake<void>(X + 8); });
    args_case(e + ": x_row_stride + 4 -> LA_ERR_STRIDE", b, fn, [](A& a) { a.x_row_stride += 4; });
    args_case(e + ": x_batch_stride negative -> LA_ERR_STRIDE", b, fn, [](A& a) { a.x_batch_stride = -51200; });
    args_case(e + ": x_head_stride 2^29 (32-bit chunk offset) -> LA_ERR_STRIDE", b, fn, [](A& a) { a.x_head_stride = 1 << 29; });
    args_case(e + ": fp32 x_row_stride + 4 -> passes (4 fp32 elements are 16 bytes)", b, fn, [](A& a) { a.in_dtype = FP32; a.x_row_stride += 4; });
    args_case(e + ": out_head_stride + 4 -> LA_ERR_STRIDE", b, fn, [](A& a) { a.out_head_stride += 4; });
    args_case(e + ": out + 4 bytes -> LA_ERR_STRIDE", b, fn, [](A& a) { a.out = fake<void>(OUT + 4); });
    args_case(e + ": x_batch_stride + 4 with batch 1 -> passes (unused stride)", b, fn, [](A& a) { a.batch = 1; a.x_batch_stride += 4; });
    args_case(e + ": weight + 8 bytes -> LA_ERR_STRIDE", b, fn, [](A& a) { a.weight = fake<float>(0x50000008); });
    args_case(e + ": rope_table[1] + 4 bytes -> LA_ERR_STRIDE", b, fn, [](A& a) { a.rope_table[1] = fake<float>(0x52000004); });
    args_case(e + ": axis_pairs[2] -1 -> LA_ERR_SHAPE", b, fn, [](A& a) { a.axis_pairs[2] = -1; });
    args_case(e + ": 65 pairs at head_dim 128 -> LA_ERR_SHAPE", b, fn, [](A& a) { a.axis_pairs[0] = 17; });
    args_case(e + ": pos_offset -1 -> LA_ERR_SHAPE", b, fn, [](A& a) { a.pos_offset = -1; });
    args_case(e + ": rope_table[0] NULL with pairs -> LA_ERR_NULL_ARG", b, fn, [](A& a) { a.rope_table[0] = nullptr; });
    args_case(e + ": axis_extent[1] 0 -> LA_ERR_SHAPE", b, fn, [](A& a) { a.axis_extent[1] = 0; });
    args_case(e + ": axis_extent 65536 x 65536 -> LA_ERR_SHAPE (first two)", b, fn, [](A& a) { a.axis_extent[0] = a.axis_extent[1] = 65536; });
    args_case(e + ": axis_extent 65536 x 4 x 65536 -> LA_ERR_SHAPE (all three)", b, fn, [](A& a) { a.axis_extent[0] = a.axis_extent[2] = 65536; a.axis_extent[1] = 4; });
    args_case(e + ": pos_offset 1 + seqlen 100 on 100 positions -> LA_ERR_SHAPE", b, fn, [](A& a) { a.pos_offset = 1; });
    args_case(e + ": all tables NULL -> no rotation, pairs 0", b, fn, [](A& a) { a.rope_table[0] = a.rope_table[1] = a.rope_table[2] = nullptr; a.axis_extent[0] = 0; });
    args_case(e + ": LA_NORM_NONE -> weight not handed on", b, fn, [](A& a) { a.norm_mode = LA_NORM_NONE; });
}

void cases_other_entry_points() {
    // la_get_tile_sizes_ex / la_get_tile_sizes / la_device_slots
    const auto tiles = [](const std::string& name, int d, int es, uint32_t flags) {
        int bm = -1, bn = -1;
        const int rc = la_get_tile_sizes_ex(d, es, flags, &bm, &bn);
        run_case("la_get_tile_sizes_ex: " + name, [&]() -> int64_t { return rc; }, {}, ",\"block_m\":" + std::to_string(bm) + ",\"block_n\":" + std::to_string(bn));
    };
    for (int es : {2, 1})
        for (int d : {64, 96, 128, 192, 256})
            for (uint32_t fl : {0u, LA_FLAG_KERNEL_128ROW, LA_FLAG_HALF_VOTE, LA_FLAG_HALF_VOTE | LA_FLAG_KERNEL_128ROW})
                tiles("d" + std::to_string(d) + " element size " + std::to_string(es) + " flags " + std::to_string(fl), d, es, fl);
    tiles("head_dim 80 -> LA_ERR_HEAD_DIM", 80, 2, 0);
    tiles("element size 4 -> LA_ERR_DTYPE", 128, 4, 0);
    tiles("flag 256 -> LA_ERR_UNSUPPORTED", 128, 2, 256u);
    run_case("la_get_tile_sizes_ex: NULL outputs -> LA_OK", [&]() -> int64_t { return la_get_tile_sizes_ex(128, 2, 0, nullptr, nullptr); });
    run_case("la_get_tile_sizes: d128 bf16", [&]() -> int64_t { int bm = 0, bn = 0; const int rc = la_get_tile_sizes(128, 2, &bm, &bn); return rc ? rc : bm * 1000 + bn; });
    const auto slots = [](const std::string& name, int d, int es, uint32_t flags) {
        int cu = -1, wg = -1;
        const int rc = la_device_slots(d, es, flags, &cu, &wg);
        run_case("la_device_slots: " + name, [&]() -> int64_t { return rc; }, {}, ",\"compute_units\":" + std::to_string(cu) + ",\"workgroups_per_cu\":" + std::to_string(wg));
    };
    slots("d128 bf16", 128, 2, 0);
    slots("d128 bf16 LA_FLAG_KERNEL_128ROW -> 2 per CU", 128, 2, LA_FLAG_KERNEL_128ROW);
    slots("d256 bf16 LA_FLAG_KERNEL_128ROW -> 1 per CU", 256, 2, LA_FLAG_KERNEL_128ROW);
    slots("d128 e4m3", 128, 1, 0);
    slots("d80 -> LA_ERR_HEAD_DIM (la_get_tile_sizes_ex)", 80, 2, 0);
    run_case("la_device_slots: NULL outputs -> LA_OK", [&]() -> int64_t { return la_device_slots(128, 2, 0, nullptr, nullptr); });

    // the list entry points: la_skip_list_stats_ex / _heads / la_skip_list_stats, la_blockmask_to_lists_ex / la_blockmask_to_lists
    const void* const list = fake<void>(RL);
    int64_t* const counts = fake<int64_t>(0x79000000);
    Knobs fail; fail.fail_at = 0; fail.fail_err = hipErrorLaunchFailure;
    using StatsFn = int (*)(const void*, int32_t, int32_t, int32_t, int32_t, int32_t, int64_t*, void*);
    for (const auto& ef : {std::pair<std::string, StatsFn>{"la_skip_list_stats_ex", la_skip_list_stats_ex}, {"la_skip_list_stats_heads", la_skip_list_stats_heads}}) {
        const std::string e = ef.first; const auto fn = ef.second;
        run_case(e + ": int32 lists", [&]() -> int64_t { return fn(list, 4, 2, 4, 3, 8, counts, STREAM); });
        run_case(e + ": int16 lists, 32766 key tiles", [&]() -> int64_t { return fn(list, 2, 2, 4, 3, 32766, counts, STREAM); });
        run_case(e + ": the launch fails -> LA_ERR_LAUNCH", [&]() -> int64_t { return fn(list, 4, 2, 4, 3, 8, counts, STREAM); }, fail);
        run_case(e + ": list NULL -> LA_ERR_NULL_ARG", [&]() -> int64_t { return fn(nullptr, 4, 2, 4, 3, 8, counts, STREAM); });
        run_case(e + ": out_counts NULL -> LA_ERR_NULL_ARG", [&]() -> int64_t { return fn(list, 4, 2, 4, 3, 8, nullptr, STREAM); });
        run_case(e + ": list_elem_size 8 -> LA_ERR_DTYPE", [&]() -> int64_t { return fn(list, 8, 2, 4, 3, 8, counts, STREAM); });
        run_case(e + ": n_batch 0 -> LA_ERR_SHAPE", [&]() -> int64_t { return fn(list, 4, 0, 4, 3, 8, counts, STREAM); });
        run_case(e + ": num_heads 0 -> LA_ERR_SHAPE", [&]() -> int64_t { return fn(list, 4, 2, 0, 3, 8, counts, STREAM); });
        run_case(e + ": q_tiles 0 -> LA_ERR_SHAPE", [&]() -> int64_t { return fn(list, 4, 2, 4, 0, 8, counts, STREAM); });
        run_case(e + ": k_tiles 0 -> LA_ERR_SHAPE", [&]() -> int64_t { return fn(list, 4, 2, 4, 3, 0, counts, STREAM); });
        run_case(e + ": int16 lists, 32767 key tiles -> LA_ERR_SEQLEN", [&]() -> int64_t { return fn(list, 2, 2, 4, 3, 32767, counts, STREAM); });
        run_case(e + ": int32 lists, 32767 key tiles -> passes", [&]() -> int64_t { return fn(list, 4, 2, 4, 3, 32767, counts, STREAM); });
        run_case(e + ": 2^31 rows -> LA_ERR_SHAPE", [&]() -> int64_t { return fn(list, 4, 65536, 32768, 1, 8, counts, STREAM); });
        run_case(e + ": 2^31 - 32768 rows -> passes", [&]() -> int64_t { return fn(list, 4, 65536, 32767, 1, 8, counts, STREAM); });
    }
    run_case("la_skip_list_stats: int32 lists (la_skip_list_stats_ex with element size 4)", [&]() -> int64_t { return la_skip_list_stats(fake<int32_t>(RL), 2, 4, 3, 8, counts, STREAM); });
    run_case("la_skip_list_stats: list NULL -> LA_ERR_NULL_ARG", [&]() -> int64_t { return la_skip_list_stats(nullptr, 2, 4, 3, 8, counts, STREAM); });
    const uint8_t* const mask = fake<uint8_t>(0x7a000000);
    const int32_t* const qv = fake<int32_t>(0x7b000000); const int32_t* const kv = fake<int32_t>(0x7c000000);
    int32_t* const empty = fake<int32_t>(0x7d000000);
    const auto bm2l = [&](const std::string& name, const uint8_t* m, int64_t mbs, int64_t mhs, int b, int h, int qt, int kt, void* l, int es, const Knobs& kn = {}) {
        run_case("la_blockmask_to_lists_ex: " + name, [&]() -> int64_t { return la_blockmask_to_lists_ex(m, mbs, mhs, b, h, qt, kt, qv, kv, l, es, empty, STREAM); }, kn);
    };
    void* const lists = fake<void>(WL);
    bm2l("int32 lists", mask, 96, 24, 2, 4, 3, 8, lists, 4);
    bm2l("int16 lists, one mask for all", mask, 0, 0, 2, 4, 3, 8, lists, 2);
    bm2l("the launch fails -> LA_ERR_LAUNCH", mask, 96, 24, 2, 4, 3, 8, lists, 4, fail);
    bm2l("blockmask NULL -> LA_ERR_NULL_ARG", nullptr, 96, 24, 2, 4, 3, 8, lists, 4);
    bm2l("lists NULL -> LA_ERR_NULL_ARG", mask, 96, 24, 2, 4, 3, 8, nullptr, 4);
    bm2l("list_elem_size 1 -> LA_ERR_DTYPE", mask, 96, 24, 2, 4, 3, 8, lists, 1);
    bm2l("batch 0 -> LA_ERR_SHAPE", mask, 96, 24, 0, 4, 3, 8, lists, 4);
    bm2l("k_tiles -1 -> LA_ERR_SHAPE", mask, 96, 24, 2, 4, 3, -1, lists, 4);
    bm2l("int16 lists, 32767 key tiles -> LA_ERR_SEQLEN", mask, 96, 24, 2, 4, 3, 32767, lists, 2);
    bm2l("int16 lists, 32767 key tiles and a negative stride -> LA_ERR_SEQLEN first", mask, -96, 24, 2, 4, 3, 32767, lists, 2);
    bm2l("mask_batch_stride -96 -> LA_ERR_STRIDE", mask, -96, 24, 2, 4, 3, 8, lists, 4);
    bm2l("mask_head_stride -24 -> LA_ERR_STRIDE", mask, 96, -24, 2, 4, 3, 8, lists, 4);
    bm2l("2^31 rows -> LA_ERR_SHAPE", mask, 0, 0, 65536, 32768, 1, 8, lists, 4);
    bm2l("2^31 rows and a negative stride -> LA_ERR_STRIDE first", mask, 0, -1, 65536, 32768, 1, 8, lists, 4);
    run_case("la_blockmask_to_lists: int32 lists (the _ex form with element size 4), no valid counts", [&]() -> int64_t {
        return la_blockmask_to_lists(mask, 96, 24, 2, 4, 3, 8, nullptr, nullptr, fake<int32_t>(WL), nullptr, STREAM); });
    run_case("la_blockmask_to_lists: lists NULL -> LA_ERR_NULL_ARG", [&]() -> int64_t {
        return la_blockmask_to_lists(mask, 96, 24, 2, 4, 3, 8, qv, kv, nullptr, empty, STREAM); });

    // la_combine / la_combine_list
    const void* const op = fake<void>(0x61000000); const float* const lp = fake<float>(0x62000000);
    void* const o = fake<void>(O); float* const lse = fake<float>(LSE);
    const auto comb = [&](const std::string& name, const void* opart, int is16, const float* lpart, void* out, int dt, int n, int b, int s, int h, int d, const Knobs& kn = {}) {
        run_case("la_combine: " + name, [&]() -> int64_t { return la_combine(opart, is16, lpart, out, dt, lse, n, b, s, h, d, STREAM); }, kn);
    };
    comb("fp32 partials -> bf16", op, 0, lp, o, BF16, 3, 2, 131, 4, 128);
    comb("16-bit partials -> fp16", op, 1, lp, o, FP16, 3, 2, 131, 4, 128);
    comb("fp32 partials -> fp32", op, 0, lp, o, FP32, 3, 2, 131, 4, 128);
    comb("the launch fails -> LA_ERR_LAUNCH", op, 0, lp, o, BF16, 3, 2, 131, 4, 128, fail);
    comb("o_partial NULL -> LA_ERR_NULL_ARG", nullptr, 0, lp, o, BF16, 3, 2, 131, 4, 128);
    comb("lse_partial NULL -> LA_ERR_NULL_ARG", op, 0, nullptr, o, BF16, 3, 2, 131, 4, 128);
    comb("o NULL -> LA_ERR_NULL_ARG", op, 0, lp, nullptr, BF16, 3, 2, 131, 4, 128);
    comb("o_dtype e4m3 -> LA_ERR_DTYPE", op, 0, lp, o, E4M3, 3, 2, 131, 4, 128);
    comb("fp32 result of 16-bit partials -> LA_ERR_DTYPE", op, 1, lp, o, FP32, 3, 2, 131, 4, 128);
    comb("num_splits 0 -> LA_ERR_SHAPE", op, 0, lp, o, BF16, 0, 2, 131, 4, 128);
    comb("seqlen_q 0 -> LA_ERR_SHAPE", op, 0, lp, o, BF16, 3, 2, 0, 4, 128);
    comb("num_splits 9 -> passes (no list limit)", op, 0, lp, o, BF16, 9, 2, 131, 4, 128);
    comb("head_dim_v 100 -> LA_ERR_HEAD_DIM", op, 0, lp, o, BF16, 3, 2, 131, 4, 100);
    comb("o_partial + 8 bytes -> LA_ERR_STRIDE", fake<void>(0x61000008), 0, lp, o, BF16, 3, 2, 131, 4, 128);
    comb("o + 8 bytes -> LA_ERR_STRIDE", op, 0, lp, fake<void>(O + 8), BF16, 3, 2, 131, 4, 128);
    const void* ops[9]; const float* lps[9];
    const auto reset_lists = [&]() { for (int i = 0; i < 9; ++i) { ops[i] = fake<void>(0x61000000 + 0x100000 * i); lps[i] = fake<float>(0x62000000 + 0x100000 * i); } };
    const auto combl = [&](const std::string& name, const void* const* opl, int is16, const float* const* lpl, void* out, int dt, int n, int b, int s, int h, int d, const Knobs& kn = {}) {
        run_case("la_combine_list: " + name, [&]() -> int64_t { return la_combine_list(opl, is16, lpl, out, dt, lse, n, b, s, h, d, STREAM); }, kn);
    };
    reset_lists();
    combl("fp32 partials -> bf16", ops, 0, lps, o, BF16, 3, 2, 131, 4, 128);
    combl("16-bit partials -> fp16, 8 splits", ops, 1, lps, o, FP16, 8, 2, 131, 4, 128);
    combl("fp32 partials -> fp32", ops, 0, lps, o, FP32, 2, 2, 131, 4, 128);
    combl("the launch fails -> LA_ERR_LAUNCH", ops, 0, lps, o, BF16, 3, 2, 131, 4, 128, fail);
    combl("o_partials NULL -> LA_ERR_NULL_ARG", nullptr, 0, lps, o, BF16, 3, 2, 131, 4, 128);
    combl("lse_partials NULL -> LA_ERR_NULL_ARG", ops, 0, nullptr, o, BF16, 3, 2, 131, 4, 128);
    combl("o NULL -> LA_ERR_NULL_ARG", ops, 0, lps, nullptr, BF16, 3, 2, 131, 4, 128);
    combl("o_dtype e4m3 -> LA_ERR_DTYPE", ops, 0, lps, o, E4M3, 3, 2, 131, 4, 128);
    combl("fp32 result of 16-bit partials -> LA_ERR_DTYPE", ops, 1, lps, o, FP32, 3, 2, 131, 4, 128);
    combl("num_splits 0 -> LA_ERR_SHAPE", ops, 0, lps, o, BF16, 0, 2, 131, 4, 128);
    combl("num_splits 9 -> LA_ERR_SHAPE (LA_COMBINE_LIST_MAX)", ops, 0, lps, o, BF16, 9, 2, 131, 4, 128);
    combl("batch 0 -> LA_ERR_SHAPE", ops, 0, lps, o, BF16, 3, 0, 131, 4, 128);
    combl("head_dim_v 100 -> LA_ERR_HEAD_DIM", ops, 0, lps, o, BF16, 3, 2, 131, 4, 100);
    combl("o + 8 bytes -> LA_ERR_STRIDE", ops, 0, lps, fake<void>(O + 8), BF16, 3, 2, 131, 4, 128);
    ops[1] = nullptr;
    combl("o_partials[1] NULL -> LA_ERR_NULL_ARG", ops, 0, lps, o, BF16, 3, 2, 131, 4, 128);
    reset_lists(); lps[2] = nullptr;
    combl("lse_partials[2] NULL -> LA_ERR_NULL_ARG", ops, 0, lps, o, BF16, 3, 2, 131, 4, 128);
    reset_lists(); ops[2] = fake<void>(0x61200008);
    combl("o_partials[2] + 8 bytes -> LA_ERR_STRIDE", ops, 0, lps, o, BF16, 3, 2, 131, 4, 128);
    combl("o_partials[2] + 8 bytes behind num_splits 2 -> passes", ops, 0, lps, o, BF16, 2, 2, 131, 4, 128);

    // la_output_error
    struct OE { const void* out; int od; int64_t obs, ors, ohs; const void* ref; int rd; int64_t rbs, rrs, rhs; int b, s, h, d, rpb; double* stats; };
    const OE oe{fake<void>(OUT), BF16, 131 * 512, 512, 128, fake<void>(X), FP32, 131 * 512, 512, 128, 2, 131, 4, 128, 64, fake<double>(0x7e000000)};
    const auto oerr = [&](const std::string& name, const std::function<void(OE&)>& m, const Knobs& kn = {}) {
        OE a = oe;
        m(a);
        run_case("la_output_error: " + name, [&]() -> int64_t {
            return la_output_error(a.out, a.od, a.obs, a.ors, a.ohs, a.ref, a.rd, a.rbs, a.rrs, a.rhs, a.b, a.s, a.h, a.d, a.rpb, a.stats, STREAM); }, kn);
    };
    oerr("bf16 against fp32", [](OE&) {});
    oerr("the launch fails -> LA_ERR_LAUNCH", [](OE&) {}, fail);
    oerr("out NULL -> LA_ERR_NULL_ARG", [](OE& a) { a.out = nullptr; });
    oerr("ref NULL -> LA_ERR_NULL_ARG", [](OE& a) { a.ref = nullptr; });
    oerr("stats NULL -> LA_ERR_NULL_ARG", [](OE& a) { a.stats = nullptr; });
    oerr("out_dtype e4m3 -> LA_ERR_DTYPE", [](OE& a) { a.od = E4M3; });
    oerr("ref_dtype 4 -> LA_ERR_DTYPE", [](OE& a) { a.rd = 4; });
    oerr("rows_per_bin 0 -> LA_ERR_SHAPE", [](OE& a) { a.rpb = 0; });
    oerr("num_heads 0 -> LA_ERR_SHAPE", [](OE& a) { a.h = 0; });
    oerr("head_dim 100 -> LA_ERR_HEAD_DIM", [](OE& a) { a.d = 100; });
    oerr("out + 8 bytes -> LA_ERR_STRIDE", [](OE& a) { a.out = fake<void>(OUT + 8); });
    oerr("out_row_stride + 4 (bf16) -> LA_ERR_STRIDE", [](OE& a) { a.ors += 4; });
    oerr("ref_row_stride + 4 (fp32) -> passes", [](OE& a) { a.rrs += 4; });
    oerr("ref_head_stride + 2 (fp32) -> LA_ERR_STRIDE", [](OE& a) { a.rhs += 2; });
    oerr("ref_batch_stride negative -> LA_ERR_STRIDE", [](OE& a) { a.rbs = -a.rbs; });
    oerr("out_batch_stride + 4 with batch 2 -> LA_ERR_STRIDE", [](OE& a) { a.obs += 4; });
    oerr("out_batch_stride + 4 with batch 1 -> passes (unused stride)", [](OE& a) { a.obs += 4; a.b = 1; });
    oerr("out_row_stride + 4 with seqlen 1 -> LA_ERR_STRIDE (the row stride is checked even when unused)", [](OE& a) { a.ors += 4; a.s = 1; });
    oerr("out_head_stride + 4 with one head -> LA_ERR_STRIDE (the head stride is checked even when unused)", [](OE& a) { a.ohs += 4; a.h = 1; });
    oerr("65536 x 32768 bins -> LA_ERR_SHAPE", [](OE& a) { a.b = 65536; a.h = 32768; a.s = 64; });

    // la_qk_prep, la_qk_prep_fp8, la_qk_prep_smooth (+ _parts, _part_rows), la_colsum_finish
    const la_qk_prep_args qp = with(prep_base<la_qk_prep_args>(), [](la_qk_prep_args& a) { a.out_dtype = FP16; });
    const std::string e0 = "la_qk_prep";
    run_case(e0 + ": NULL args -> LA_ERR_NULL_ARG", [&]() -> int64_t { return la_qk_prep(nullptr, STREAM); });
    args_case(e0 + ": bf16 -> fp16, LA_NORM_TOKEN, rope", qp, la_qk_prep, keep);
    args_case(e0 + ": the launch fails -> LA_ERR_LAUNCH", qp, la_qk_prep, keep, fail);
    args_case(e0 + ": struct_size + 8 -> LA_ERR_STRUCT_SIZE", qp, la_qk_prep, [](la_qk_prep_args& a) { a.struct_size += 8; });
    args_case(e0 + ": x NULL -> LA_ERR_NULL_ARG", qp, la_qk_prep, [](la_qk_prep_args& a) { a.x = nullptr; });
    args_case(e0 + ": out NULL -> LA_ERR_NULL_ARG", qp, la_qk_prep, [](la_qk_prep_args& a) { a.out = nullptr; });
    args_case(e0 + ": in_dtype e4m3 -> LA_ERR_DTYPE", qp, la_qk_prep, [](la_qk_prep_args& a) { a.in_dtype = E4M3; });
    args_case(e0 + ": out_dtype fp32 -> LA_ERR_DTYPE", qp, la_qk_prep, [](la_qk_prep_args& a) { a.out_dtype = FP32; });
    args_case(e0 + ": in_dtype fp32 -> passes", qp, la_qk_prep, [](la_qk_prep_args& a) { a.in_dtype = FP32; });
    cases_prep_shared(e0, qp, la_qk_prep);

    const la_qk_prep_fp8_args q8 = with(prep_base<la_qk_prep_fp8_args>(), [](la_qk_prep_fp8_args& a) { scale_fields(a); });
    const std::string e1 = "la_qk_prep_fp8";
    using A8 = la_qk_prep_fp8_args;
    run_case(e1 + ": NULL args -> LA_ERR_NULL_ARG", [&]() -> int64_t { return la_qk_prep_fp8(nullptr, STREAM); });
    args_case(e1 + ": quantize (mode 1)", q8, la_qk_prep_fp8, keep);
    args_case(e1 + ": out NULL -> the amax pass (mode 2), descale not handed on", q8, la_qk_prep_fp8, [](A8& a) { a.out = nullptr; });
    args_case(e1 + ": the launch fails -> LA_ERR_LAUNCH", q8, la_qk_prep_fp8, keep, fail);
    args_case(e1 + ": struct_size 0 -> LA_ERR_STRUCT_SIZE", q8, la_qk_prep_fp8, [](A8& a) { a.struct_size = 0; });
    args_case(e1 + ": x NULL -> LA_ERR_NULL_ARG", q8, la_qk_prep_fp8, [](A8& a) { a.x = nullptr; });
    args_case(e1 + ": out and amax NULL -> LA_ERR_NULL_ARG", q8, la_qk_prep_fp8, [](A8& a) { a.out = nullptr; a.amax = nullptr; });
    args_case(e1 + ": in_dtype e4m3 -> LA_ERR_DTYPE", q8, la_qk_prep_fp8, [](A8& a) { a.in_dtype = E4M3; });
    args_case(e1 + ": heads_per_scale 0 -> LA_ERR_SHAPE", q8, la_qk_prep_fp8, [](A8& a) { a.heads_per_scale = 0; });
    args_case(e1 + ": heads_per_scale 3 of 4 heads -> LA_ERR_SHAPE", q8, la_qk_prep_fp8, [](A8& a) { a.heads_per_scale = 3; });
    args_case(e1 + ": num_heads 0 -> LA_ERR_SHAPE (scale groups)", q8, la_qk_prep_fp8, [](A8& a) { a.num_heads = 0; });
    args_case(e1 + ": descale_batch_stride -2 -> LA_ERR_STRIDE", q8, la_qk_prep_fp8, [](A8& a) { a.descale_batch_stride = -2; });
    args_case(e1 + ": amax_head_stride -1 -> LA_ERR_STRIDE", q8, la_qk_prep_fp8, [](A8& a) { a.amax_head_stride = -1; });
    args_case(e1 + ": amax + 2 bytes -> LA_ERR_STRIDE", q8, la_qk_prep_fp8, [](A8& a) { a.amax = fake<float>(0x55000002); });
    args_case(e1 + ": out + 8 bytes -> passes (8-byte rows of e4m3)", q8, la_qk_prep_fp8, [](A8& a) { a.out = fake<void>(OUT + 8); });
    args_case(e1 + ": 1026 heads -> LA_ERR_UNSUPPORTED (scale slots)", q8, la_qk_prep_fp8, [](A8& a) { a.num_heads = 1026; a.norm_mode = LA_NORM_HEAD; });
    args_case(e1 + ": 1024 heads -> passes", q8, la_qk_prep_fp8, [](A8& a) { a.num_heads = 1024; a.norm_mode = LA_NORM_HEAD; });
    cases_prep_shared(e1, q8, la_qk_prep_fp8);

    using AS = la_qk_prep_smooth_args;
    const AS qs = with(prep_base<AS>(), [](AS& a) {
        scale_fields(a);
        a.shift = fake<float>(0x56000000); a.shift_batch_stride = 512; a.shift_head_stride = 128;
        a.colsum_part = fake<float>(0x57000000);
        a.dot_vec = fake<float>(0x58000000); a.dot_vec_batch_stride = 256; a.dot_vec_head_stride = 128; a.heads_per_dot = 2;
        a.dot_out = fake<float>(0x59000000);
    });
    const std::string e2 = "la_qk_prep_smooth";
    run_case(e2 + ": NULL args -> LA_ERR_NULL_ARG", [&]() -> int64_t { return la_qk_prep_smooth(nullptr, STREAM); });
    args_case(e2 + ": shift, column sums and dots (mode 3)", qs, la_qk_prep_smooth, keep);
    args_case(e2 + ": the same without out (mode 4)", qs, la_qk_prep_smooth, [](AS& a) { a.out = nullptr; });
    args_case(e2 + ": nothing added -> la_qk_prep_fp8's mode 1", qs, la_qk_prep_smooth, [](AS& a) { a.shift = nullptr; a.colsum_part = nullptr; a.dot_vec = nullptr; a.dot_out = nullptr; });
    args_case(e2 + ": column sums alone, no out (mode 4)", qs, la_qk_prep_smooth, [](AS& a) { a.out = nullptr; a.amax = nullptr; a.shift = nullptr; a.dot_vec = nullptr; a.dot_out = nullptr; });
    args_case(e2 + ": the launch fails -> LA_ERR_LAUNCH", qs, la_qk_prep_smooth, keep, fail);
    args_case(e2 + ": struct_size 0 -> LA_ERR_STRUCT_SIZE", qs, la_qk_prep_smooth, [](AS& a) { a.struct_size = 0; });
    args_case(e2 + ": x NULL -> LA_ERR_NULL_ARG", qs, la_qk_prep_smooth, [](AS& a) { a.x = nullptr; });
    args_case(e2 + ": no output at all -> LA_ERR_NULL_ARG", qs, la_qk_prep_smooth, [](AS& a) { a.out = nullptr; a.amax = nullptr; a.colsum_part = nullptr; a.dot_out = nullptr; a.dot_vec = nullptr; });
    args_case(e2 + ": dot_out without dot_vec -> LA_ERR_NULL_ARG", qs, la_qk_prep_smooth, [](AS& a) { a.dot_vec = nullptr; });
    args_case(e2 + ": dot_vec without dot_out -> LA_ERR_NULL_ARG", qs, la_qk_prep_smooth, [](AS& a) { a.dot_out = nullptr; });
    args_case(e2 + ": in_dtype e4m3 -> LA_ERR_DTYPE", qs, la_qk_prep_smooth, [](AS& a) { a.in_dtype = E4M3; });
    args_case(e2 + ": heads_per_scale 3 -> LA_ERR_SHAPE", qs, la_qk_prep_smooth, [](AS& a) { a.heads_per_scale = 3; });
    args_case(e2 + ": heads_per_dot 0 -> LA_ERR_SHAPE", qs, la_qk_prep_smooth, [](AS& a) { a.heads_per_dot = 0; });
    args_case(e2 + ": heads_per_dot 3 -> LA_ERR_SHAPE", qs, la_qk_prep_smooth, [](AS& a) { a.heads_per_dot = 3; });
    args_case(e2 + ": heads_per_dot 0 without dot_vec -> passes", qs, la_qk_prep_smooth, [](AS& a) { a.heads_per_dot = 0; a.dot_vec = nullptr; a.dot_out = nullptr; });
    args_case(e2 + ": descale_head_stride -1 -> LA_ERR_STRIDE", qs, la_qk_prep_smooth, [](AS& a) { a.descale_head_stride = -1; });
    args_case(e2 + ": dot_out + 2 bytes -> LA_ERR_STRIDE", qs, la_qk_prep_smooth, [](AS& a) { a.dot_out = fake<float>(0x59000002); });
    args_case(e2 + ": shift + 8 bytes -> LA_ERR_STRIDE", qs, la_qk_prep_smooth, [](AS& a) { a.shift = fake<float>(0x56000008); });
    args_case(e2 + ": shift_head_stride + 2 -> LA_ERR_STRIDE", qs, la_qk_prep_smooth, [](AS& a) { a.shift_head_stride += 2; });
    args_case(e2 + ": dot_vec_batch_stride negative -> LA_ERR_STRIDE", qs, la_qk_prep_smooth, [](AS& a) { a.dot_vec_batch_stride = -256; });
    args_case(e2 + ": dot_vec_head_stride + 2 with one group -> passes (unused stride)", qs, la_qk_prep_smooth, [](AS& a) { a.dot_vec_head_stride += 2; a.heads_per_dot = 4; });
    args_case(e2 + ": colsum_part + 8 bytes -> LA_ERR_STRIDE", qs, la_qk_prep_smooth, [](AS& a) { a.colsum_part = fake<float>(0x57000008); });
    args_case(e2 + ": 1026 heads -> LA_ERR_UNSUPPORTED (scale slots)", qs, la_qk_prep_smooth, [](AS& a) { a.num_heads = 1026; a.norm_mode = LA_NORM_HEAD; });
    Knobs s16; s16.sum_slots = 16;
    Knobs s17; s17.sum_slots = 17;
    args_case(e2 + ": 17 column-sum slots -> LA_ERR_UNSUPPORTED", qs, la_qk_prep_smooth, keep, s17);
    args_case(e2 + ": 16 column-sum slots -> passes", qs, la_qk_prep_smooth, keep, s16);
    args_case(e2 + ": 17 column-sum slots without colsum_part -> passes", qs, la_qk_prep_smooth, [](AS& a) { a.colsum_part = nullptr; }, s17);
    cases_prep_shared(e2, qs, la_qk_prep_smooth);
    using Fn3 = int (*)(int32_t, int32_t, int32_t);
    for (const auto& ef : {std::pair<std::string, Fn3>{"la_qk_prep_smooth_parts", la_qk_prep_smooth_parts}, {"la_qk_prep_smooth_part_rows", la_qk_prep_smooth_part_rows},
                                {"la_v_colstats_parts", la_v_colstats_parts}, {"la_v_colstats_part_rows", la_v_colstats_part_rows}}) {
        const std::string e = ef.first; const auto fn = ef.second;
        run_case(e + ": (75600, 40, 128)", [&]() -> int64_t { return fn(75600, 40, 128); });
        run_case(e + ": (100, 4, 128)", [&]() -> int64_t { return fn(100, 4, 128); });
        run_case(e + ": seqlen 0 -> LA_ERR_SHAPE", [&]() -> int64_t { return fn(0, 4, 128); });
        run_case(e + ": num_heads 0 -> LA_ERR_SHAPE", [&]() -> int64_t { return fn(100, 0, 128); });
        run_case(e + ": head_dim -1 -> LA_ERR_SHAPE", [&]() -> int64_t { return fn(100, 4, -1); });
    }
    const float* const part = fake<float>(0x57000000); float* const mean = fake<float>(0x5a000000); float* const amax = fake<float>(0x5b000000);
    const auto csf = [&](const std::string& name, const float* p, int n, int b, int h, int d, int s, float* m, int64_t mbs, int64_t mhs, const Knobs& kn = {}) {
        run_case("la_colsum_finish: " + name, [&]() -> int64_t { return la_colsum_finish(p, n, b, h, d, s, m, mbs, mhs, STREAM); }, kn);
    };
    csf("4 parts", part, 4, 2, 4, 128, 100, mean, 512, 128);
    csf("the launch fails -> LA_ERR_LAUNCH", part, 4, 2, 4, 128, 100, mean, 512, 128, fail);
    csf("part NULL -> LA_ERR_NULL_ARG", nullptr, 4, 2, 4, 128, 100, mean, 512, 128);
    csf("mean_out NULL -> LA_ERR_NULL_ARG", part, 4, 2, 4, 128, 100, nullptr, 512, 128);
    csf("n_parts 0 -> LA_ERR_SHAPE", part, 0, 2, 4, 128, 100, mean, 512, 128);
    csf("seqlen 0 -> LA_ERR_SHAPE", part, 4, 2, 4, 128, 0, mean, 512, 128);
    csf("mean_batch_stride -512 -> LA_ERR_STRIDE", part, 4, 2, 4, 128, 100, mean, -512, 128);
    csf("mean_out + 2 bytes -> LA_ERR_STRIDE", part, 4, 2, 4, 128, 100, fake<float>(0x5a000002), 512, 128);
    csf("2^31 x 2^9 columns -> LA_ERR_SHAPE", part, 4, 1 << 20, 1 << 12, 1 << 8, 100, mean, 512, 128);

    // la_v_colstats (+ _finish), la_attn_unshift
    using AV = la_v_colstats_args;
    AV vc;
    memset(&vc, 0, sizeof vc);
    vc.struct_size = sizeof vc; vc.in_dtype = BF16; vc.x = fake<void>(X); vc.stat_part = fake<float>(0x57000000);
    vc.batch = 2; vc.seqlen = 100; vc.num_heads = 4; vc.head_dim = 128; vc.x_head_stride = 128; vc.x_row_stride = 512; vc.x_batch_stride = 51200;
    const std::string e3 = "la_v_colstats";
    run_case(e3 + ": NULL args -> LA_ERR_NULL_ARG", [&]() -> int64_t { return la_v_colstats(nullptr, STREAM); });
    args_case(e3 + ": bf16", vc, la_v_colstats, keep);
    args_case(e3 + ": fp32, 75600 rows", vc, la_v_colstats, [](AV& a) { a.in_dtype = FP32; a.seqlen = 75600; });
    args_case(e3 + ": the launch fails -> LA_ERR_LAUNCH", vc, la_v_colstats, keep, fail);
    args_case(e3 + ": struct_size 0 -> LA_ERR_STRUCT_SIZE", vc, la_v_colstats, [](AV& a) { a.struct_size = 0; });
    args_case(e3 + ": x NULL -> LA_ERR_NULL_ARG", vc, la_v_colstats, [](AV& a) { a.x = nullptr; });
    args_case(e3 + ": stat_part NULL -> LA_ERR_NULL_ARG", vc, la_v_colstats, [](AV& a) { a.stat_part = nullptr; });
    args_case(e3 + ": in_dtype e4m3 -> LA_ERR_DTYPE", vc, la_v_colstats, [](AV& a) { a.in_dtype = E4M3; });
    args_case(e3 + ": batch 0 -> LA_ERR_SHAPE", vc, la_v_colstats, [](AV& a) { a.batch = 0; });
    args_case(e3 + ": head_dim 100 -> LA_ERR_HEAD_DIM", vc, la_v_colstats, [](AV& a) { a.head_dim = 100; });
    args_case(e3 + ": head_dim 264 -> LA_ERR_HEAD_DIM", vc, la_v_colstats, [](AV& a) { a.head_dim = 264; });
    args_case(e3 + ": x_row_stride + 4 -> LA_ERR_STRIDE", vc, la_v_colstats, [](AV& a) { a.x_row_stride += 4; });
    args_case(e3 + ": x_row_stride + 4 with seqlen 1 -> passes (unused stride)", vc, la_v_colstats, [](AV& a) { a.x_row_stride += 4; a.seqlen = 1; });
    args_case(e3 + ": stat_part + 8 bytes -> LA_ERR_STRIDE", vc, la_v_colstats, [](AV& a) { a.stat_part = fake<float>(0x57000008); });
    args_case(e3 + ": 2^31 x 2^9 threads -> LA_ERR_SHAPE", vc, la_v_colstats, [](AV& a) { a.batch = 1 << 20; a.num_heads = 1 << 16; a.head_dim = 256; a.seqlen = 16; });
    const auto vcf = [&](const std::string& name, const float* p, int n, int b, int h, int d, int s, float* m, int64_t mbs, int64_t mhs, float* am, int64_t abs_, int64_t ahs, const Knobs& kn = {}) {
        run_case("la_v_colstats_finish: " + name, [&]() -> int64_t { return la_v_colstats_finish(p, n, b, h, d, s, m, mbs, mhs, am, abs_, ahs, STREAM); }, kn);
    };
    vcf("4 parts", part, 4, 2, 4, 128, 100, mean, 512, 128, amax, 4, 1);
    vcf("no amax", part, 4, 2, 4, 128, 100, mean, 512, 128, nullptr, 0, 0);
    vcf("the launch fails -> LA_ERR_LAUNCH", part, 4, 2, 4, 128, 100, mean, 512, 128, amax, 4, 1, fail);
    vcf("part NULL -> LA_ERR_NULL_ARG", nullptr, 4, 2, 4, 128, 100, mean, 512, 128, amax, 4, 1);
    vcf("mean_out NULL -> LA_ERR_NULL_ARG", part, 4, 2, 4, 128, 100, nullptr, 512, 128, amax, 4, 1);
    vcf("num_heads 0 -> LA_ERR_SHAPE", part, 4, 2, 0, 128, 100, mean, 512, 128, amax, 4, 1);
    vcf("head_dim 264 -> LA_ERR_HEAD_DIM", part, 4, 2, 4, 264, 100, mean, 512, 128, amax, 4, 1);
    vcf("amax_head_stride -1 -> LA_ERR_STRIDE", part, 4, 2, 4, 128, 100, mean, 512, 128, amax, 4, -1);
    vcf("amax_out + 2 bytes -> LA_ERR_STRIDE", part, 4, 2, 4, 128, 100, mean, 512, 128, fake<float>(0x5b000002), 4, 1);
    vcf("65536 x 32768 heads -> LA_ERR_SHAPE", part, 4, 65536, 32768, 128, 100, mean, 512, 128, amax, 4, 1);
    using AU = la_attn_unshift_args;
    AU au;
    memset(&au, 0, sizeof au);
    au.struct_size = sizeof au; au.o_dtype = BF16; au.out_dtype = FP32; au.heads_per_vec = 2; au.o = fake<void>(O); au.out = fake<void>(OUT);
    au.batch = 2; au.seqlen = 100; au.num_heads = 4; au.head_dim = 128;
    au.o_head_stride = au.out_head_stride = 128; au.o_row_stride = au.out_row_stride = 512; au.o_batch_stride = au.out_batch_stride = 51200;
    au.shift = fake<float>(0x56000000); au.shift_batch_stride = 256; au.shift_head_stride = 128;
    au.lse = fake<float>(LSE); au.lse_dot = fake<float>(0x59000000); au.lse_out = fake<float>(0x5c000000); au.softmax_scale = 0.125f;
    const std::string e4 = "la_attn_unshift";
    run_case(e4 + ": NULL args -> LA_ERR_NULL_ARG", [&]() -> int64_t { return la_attn_unshift(nullptr, STREAM); });
    args_case(e4 + ": bf16 -> fp32 with shift and LSE", au, la_attn_unshift, keep);
    args_case(e4 + ": no shift -> heads_per_vec 1", au, la_attn_unshift, [](AU& a) { a.shift = nullptr; a.heads_per_vec = 0; });
    args_case(e4 + ": the launch fails -> LA_ERR_LAUNCH", au, la_attn_unshift, keep, fail);
    args_case(e4 + ": struct_size 0 -> LA_ERR_STRUCT_SIZE", au, la_attn_unshift, [](AU& a) { a.struct_size = 0; });
    args_case(e4 + ": o NULL -> LA_ERR_NULL_ARG", au, la_attn_unshift, [](AU& a) { a.o = nullptr; });
    args_case(e4 + ": out NULL -> LA_ERR_NULL_ARG", au, la_attn_unshift, [](AU& a) { a.out = nullptr; });
    args_case(e4 + ": lse_dot without lse_out -> LA_ERR_NULL_ARG", au, la_attn_unshift, [](AU& a) { a.lse_out = nullptr; });
    args_case(e4 + ": lse_out without lse -> LA_ERR_NULL_ARG", au, la_attn_unshift, [](AU& a) { a.lse = nullptr; });
    args_case(e4 + ": o_dtype fp32 -> LA_ERR_DTYPE", au, la_attn_unshift, [](AU& a) { a.o_dtype = FP32; });
    args_case(e4 + ": out_dtype e4m3 -> LA_ERR_DTYPE", au, la_attn_unshift, [](AU& a) { a.out_dtype = E4M3; });
    args_case(e4 + ": seqlen 0 -> LA_ERR_SHAPE", au, la_attn_unshift, [](AU& a) { a.seqlen = 0; });
    args_case(e4 + ": heads_per_vec 3 -> LA_ERR_SHAPE", au, la_attn_unshift, [](AU& a) { a.heads_per_vec = 3; });
    args_case(e4 + ": head_dim 100 -> LA_ERR_HEAD_DIM", au, la_attn_unshift, [](AU& a) { a.head_dim = 100; });
    args_case(e4 + ": o_row_stride + 4 -> LA_ERR_STRIDE", au, la_attn_unshift, [](AU& a) { a.o_row_stride += 4; });
    args_case(e4 + ": out_row_stride + 4 (fp32) -> passes", au, la_attn_unshift, [](AU& a) { a.out_row_stride += 4; });
    args_case(e4 + ": out + 8 bytes -> LA_ERR_STRIDE", au, la_attn_unshift, [](AU& a) { a.out = fake<void>(OUT + 8); });
    args_case(e4 + ": shift_batch_stride + 2 -> LA_ERR_STRIDE", au, la_attn_unshift, [](AU& a) { a.shift_batch_stride += 2; });
    args_case(e4 + ": lse_dot + 2 bytes -> LA_ERR_STRIDE", au, la_attn_unshift, [](AU& a) { a.lse_dot = fake<float>(0x59000002); });

    // la_v_tiles_bytes, la_v_tiles_workspace_bytes, la_v_prep_tiles
    using Fn4 = int64_t (*)(int32_t, int32_t, int32_t, int32_t);
    for (const auto& ef : {std::pair<std::string, Fn4>{"la_v_tiles_bytes", la_v_tiles_bytes}, {"la_v_tiles_workspace_bytes", la_v_tiles_workspace_bytes}}) {
        const std::string e = ef.first; const auto fn = ef.second;
        for (int d : {64, 96, 128, 192, 256}) run_case(e + ": (2, 2, 500, " + std::to_string(d) + ")", [&]() -> int64_t { return fn(2, 2, 500, d); });
        run_case(e + ": no keys", [&]() -> int64_t { return fn(2, 2, 0, 128); });
        run_case(e + ": 413377 keys (la_fwd would cut them into runs: not this size)", [&]() -> int64_t { return fn(2, 2, 413377, 128); });
        run_case(e + ": batch 0 -> LA_ERR_SHAPE", [&]() -> int64_t { return fn(0, 2, 500, 128); });
        run_case(e + ": num_heads_k 0 -> LA_ERR_SHAPE", [&]() -> int64_t { return fn(2, 0, 500, 128); });
        run_case(e + ": seqlen_k -1 -> LA_ERR_SHAPE", [&]() -> int64_t { return fn(2, 2, -1, 128); });
        run_case(e + ": head_dim 80 -> LA_ERR_HEAD_DIM", [&]() -> int64_t { return fn(2, 2, 500, 80); });
    }
    using AT = la_v_prep_tiles_args;
    AT vt;
    memset(&vt, 0, sizeof vt);
    vt.struct_size = sizeof vt; vt.in_dtype = BF16; vt.x = fake<void>(X); vt.tiles = fake<void>(WS);
    vt.batch = 2; vt.seqlen = 500; vt.num_heads = 2; vt.head_dim = 128; vt.x_head_stride = 128; vt.x_row_stride = 256; vt.x_batch_stride = 128000;
    vt.descale = fake<float>(0x54000000); vt.descale_batch_stride = 2; vt.descale_head_stride = 1;
    vt.shift = fake<float>(0x56000000); vt.shift_batch_stride = 256; vt.shift_head_stride = 128;
    vt.amax = fake<float>(0x55000000); vt.amax_batch_stride = 2; vt.amax_head_stride = 1;
    const std::string e5 = "la_v_prep_tiles";
    run_case(e5 + ": NULL args -> LA_ERR_NULL_ARG", [&]() -> int64_t { return la_v_prep_tiles(nullptr, STREAM); });
    args_case(e5 + ": bf16 with descale, shift and amax", vt, la_v_prep_tiles, keep);
    args_case(e5 + ": fp32, nothing optional", vt, la_v_prep_tiles, [](AT& a) { a.in_dtype = FP32; a.descale = nullptr; a.shift = nullptr; a.amax = nullptr; });
    args_case(e5 + ": the launch fails -> LA_ERR_LAUNCH", vt, la_v_prep_tiles, keep, fail);
    args_case(e5 + ": struct_size 0 -> LA_ERR_STRUCT_SIZE", vt, la_v_prep_tiles, [](AT& a) { a.struct_size = 0; });
    args_case(e5 + ": x NULL -> LA_ERR_NULL_ARG", vt, la_v_prep_tiles, [](AT& a) { a.x = nullptr; });
    args_case(e5 + ": tiles NULL -> LA_ERR_NULL_ARG", vt, la_v_prep_tiles, [](AT& a) { a.tiles = nullptr; });
    args_case(e5 + ": in_dtype e4m3 -> LA_ERR_DTYPE", vt, la_v_prep_tiles, [](AT& a) { a.in_dtype = E4M3; });
    args_case(e5 + ": seqlen 0 -> LA_ERR_SHAPE", vt, la_v_prep_tiles, [](AT& a) { a.seqlen = 0; });
    args_case(e5 + ": head_dim 80 -> LA_ERR_HEAD_DIM", vt, la_v_prep_tiles, [](AT& a) { a.head_dim = 80; });
    args_case(e5 + ": reserved0 1 -> LA_ERR_UNSUPPORTED", vt, la_v_prep_tiles, [](AT& a) { a.reserved0 = 1; });
    args_case(e5 + ": x_head_stride + 4 -> LA_ERR_STRIDE", vt, la_v_prep_tiles, [](AT& a) { a.x_head_stride += 4; });
    args_case(e5 + ": shift + 8 bytes -> LA_ERR_STRIDE", vt, la_v_prep_tiles, [](AT& a) { a.shift = fake<float>(0x56000008); });
    args_case(e5 + ": tiles + 8 bytes -> LA_ERR_STRIDE", vt, la_v_prep_tiles, [](AT& a) { a.tiles = fake<void>(WS + 8); });
    args_case(e5 + ": descale_head_stride -1 -> LA_ERR_STRIDE", vt, la_v_prep_tiles, [](AT& a) { a.descale_head_stride = -1; });
    args_case(e5 + ": amax_batch_stride -2 -> LA_ERR_STRIDE", vt, la_v_prep_tiles, [](AT& a) { a.amax_batch_stride = -2; });
    args_case(e5 + ": descale + 2 bytes -> LA_ERR_STRIDE", vt, la_v_prep_tiles, [](AT& a) { a.descale = fake<float>(0x54000002); });
    args_case(e5 + ": 65536 x 32768 tiles -> LA_ERR_SHAPE", vt, la_v_prep_tiles, [](AT& a) { a.batch = 65536; a.num_heads = 32768; a.seqlen = 64; });

    // the rest of the ABI: no launch, no check
    run_case("la_abi_version", [&]() -> int64_t { return la_abi_version(); });
    for (int st = 1; st >= -14; --st)
        run_case("la_status_string(" + std::to_string(st) + ")", [&]() -> int64_t { return st; }, {}, ",\"text\":\"" + std::string(la_status_string(st)) + "\"");
}

// ---- --time N: host nanoseconds of one la_fwd call on the one-launch listed cases ------------------------------------------------------
void time_calls(long n) {
    g_timing = true;
    for (int dtype : {BF16, E4M3}) {
        const la_fwd_args a = block(dtype, 128, true);
        long ok = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (long i = 0; i < n; ++i) ok += la_fwd(&a, STREAM) == LA_OK;
        const auto t1 = std::chrono::steady_clock::now();
        printf("%s d128 lists: %.2f ns per la_fwd call (%ld of %ld calls LA_OK)\n", dname(dtype),
               std::chrono::duration<double, std::nano>(t1 - t0).count() / static_cast<double>(n), ok, n);
    }
}
}  // namespace

int main(int argc, char** argv) {
    if (argc == 3 && strcmp(argv[1], "--time") == 0) { time_calls(atol(argv[2])); return 0; }
    printf("{\"split_bounds\":{\"bf16\":{\"256\":%d,\"128\":%d},\"e4m3\":{\"256\":%d,\"64\":%d}},\n", kBoundBf16D256, kBoundBf16D128, kBoundE4m3D256, kBoundE4m3D64);
    grid_workspace_bytes();
    printf("\"cases\":[");
    cases_fwd_returns();
    cases_table_status();
    cases_launch_shapes();
    cases_split();
    cases_other_entry_points();
    printf("],\n\"legend\":{");
    bool first = true;
    for (const auto& [name, fields] : g_legend) {
        std::string f = fields;
        if (!f.empty() && f.back() == ',') f.pop_back();
        printf("%s\n\"%s\":\"%s\"", first ? "" : ",", name.c_str(), f.c_str());
        first = false;
    }
    printf("}}\n");
    return 0;
}
