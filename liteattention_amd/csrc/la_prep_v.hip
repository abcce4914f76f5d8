// la_prep_v.hip — V smoothing around the e4m3 forward: the column statistics a mean-shifted V is made from (la_v_colstats,
// la_v_colstats_finish) and the pass that puts the shift back into the attention output (la_attn_unshift). The kernel divides by its
// own row sum, so the rows of P sum to 1 over whatever keys a row visits, and P (V - 1 m^T) + 1 m^T = P V for any vector m per
// (batch, kv-head): V is quantized as V - m (la_qk_prep_smooth with LA_NORM_NONE and shift = m), the forward runs unchanged on the
// shifted codes, and m is added to O in fp32 here. HBM-bound kernels, no float atomics.
//
//  * la_v_colstats_kernel<IN>: one THREAD owns 8 consecutive columns (one 16-byte load of 16-bit elements, two of fp32) of one
//    (part, batch, head) and walks the rows [p R, min(S, (p + 1) R)) of its part: kRowsInFlight rows are loaded together, then added
//    one after the other, so the order of the additions is the order of the rows whatever the timing. It keeps 8 running sums, minima
//    and maxima in registers and writes them with six 16-byte stores: stat_part[p][0 / 1 / 2][b][h][d]. Neighbouring threads own
//    neighbouring chunks of a (batch, row): a wave reads 1 KiB of a bf16 row at once.
//    R (v_colstats_part_rows, la_kernel_params.h) = max(16, ceil(S * (H * D / 8) / 131072)): about 131072 threads - two waves per
//    SIMD of 256 compute units, each with kRowsInFlight 16-byte loads in flight (16 MiB on the way, a multiple of what the HBM
//    latency needs) - while the finish step still adds at most a few hundred parts per column. S 75 600, H D 5120: R 370, 205
//    parts, 131 200 threads. A function of (S, H, D) alone.
//    fminf / fmaxf skip a NaN; the sum does not, and the finish step makes the signal of it.
//  * la_v_colstats_finish_kernel: one workgroup per (batch, head), one thread per column: the sums of the parts added in index order
//    and divided by S, the minimum and maximum over the parts, then max(|fl(vmax - mean)|, |fl(mean - vmin)|) as bit patterns, reduced
//    over the head's columns by the xor butterfly of each wave and four words of LDS. Rounding is monotone, so this is the largest
//    |fl(x - mean)| over the rows: the bits la_qk_prep_smooth reports for shift = mean.
//  * la_attn_unshift_kernel<O, OUT>: one thread = 8 consecutive d of one (b, s, h) row, as combine_kernel; grid stride. out =
//    round(float(o) + shift[b][h / heads_per_vec][:]): one fp32 addition, one rounding at the store. A thread loads its chunk before
//    it stores it and no other thread touches that chunk, so out may be o itself.
//  * la_attn_unshift_lse_kernel<O, OUT>: the same with lse. A row whose lse is +-inf is the forward's empty sum (no weights carry the
//    shift): zeros, lse copied. o runs (s, h), lse runs (h, s): a workgroup takes a tile of 32 s x 8 heads, moves the tile's lse /
//    lse_dot / lse_out along s in whole cache lines (one element per thread, through LDS), then walks o in its own memory order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "la_kernel_params.h"
#include "la_prep_common.h"

namespace la {
namespace {

constexpr int kRowsInFlight = 8;           // rows of a thread's chunk loaded before the first of them is added
constexpr int kUnshiftMaxGrid = 8192;      // workgroups of la_attn_unshift_kernel (combine_kernel's cap); the rest by grid stride
constexpr int64_t kUnshiftMaxTiles = 1 << 20;      // ... of la_attn_unshift_lse_kernel, one tile each; more tiles by grid stride

__device__ __forceinline__ void take_row(const float (&v)[8], float (&sum)[8], float (&lo)[8], float (&hi)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        sum[j] += v[j];
        lo[j] = fminf(lo[j], v[j]);
        hi[j] = fmaxf(hi[j], v[j]);
    }
}

template <int DT>
__global__ void __launch_bounds__(256) la_v_colstats_kernel(const VColstatsParams p) {
    const int chunks = p.head_dim / 8;
    const int64_t items = static_cast<int64_t>(p.n_parts) * p.batch * p.num_heads * chunks;
    const int64_t idx = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (idx >= items) return;
    const int ch = static_cast<int>(idx % chunks);
    int64_t t = idx / chunks;                  // (part * B + b) * H + h
    const int h = static_cast<int>(t % p.num_heads);
    t /= p.num_heads;
    const int b = static_cast<int>(t % p.batch);
    const int64_t part = t / p.batch;
    const int64_t r0 = part * p.part_rows;
    const int64_t r1 = r0 + p.part_rows < p.seqlen ? r0 + p.part_rows : p.seqlen;      // r1 <= r0: a part without rows
    const int64_t col0 = b * p.x_bs + h * p.x_hs + ch * 8;
    float sum[8], lo[8], hi[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { sum[j] = 0.f; lo[j] = INFINITY; hi[j] = -INFINITY; }
    int64_t r = r0;
    for (; r + kRowsInFlight <= r1; r += kRowsInFlight) {
        typename PrepLoad<DT>::raw w[kRowsInFlight];
#pragma unroll
        for (int u = 0; u < kRowsInFlight; ++u) w[u] = PrepLoad<DT>::load(p.x, col0 + (r + u) * p.x_rs);
#pragma unroll
        for (int u = 0; u < kRowsInFlight; ++u) {
            float v[8];
            PrepLoad<DT>::to_float(w[u], v);
            take_row(v, sum, lo, hi);
        }
    }
    for (; r < r1; ++r) {
        float v[8];
        PrepLoad<DT>::to_float(PrepLoad<DT>::load(p.x, col0 + r * p.x_rs), v);
        take_row(v, sum, lo, hi);
    }
    const int64_t cols = static_cast<int64_t>(p.batch) * p.num_heads * p.head_dim;
    float* dst = p.stat_part + part * 3 * cols + (static_cast<int64_t>(b) * p.num_heads + h) * p.head_dim + ch * 8;
    PrepStore<3>::store8(dst, 0, sum);
    PrepStore<3>::store8(dst, cols, lo);
    PrepStore<3>::store8(dst, 2 * cols, hi);
}

__global__ void __launch_bounds__(256) la_v_colstats_finish_kernel(const float* __restrict__ part, int n_parts, int64_t cols, int head_dim,
                                                                     int num_heads, float seqlen, float* __restrict__ mean, int64_t m_bs,
                                                                     int64_t m_hs, float* __restrict__ amax, int64_t a_bs, int64_t a_hs) {
    __shared__ unsigned wave_max[4];
    const int64_t bh = blockIdx.x;
    const int b = static_cast<int>(bh / num_heads), h = static_cast<int>(bh - static_cast<int64_t>(b) * num_heads);
    const int d = threadIdx.x;
    unsigned m = 0;
    if (d < head_dim) {
        const float* __restrict__ src = part + bh * head_dim + d;
        float acc = 0.f, lo = INFINITY, hi = -INFINITY;
        if (amax != nullptr) {
#pragma unroll 8
            for (int q = 0; q < n_parts; ++q) {
                acc += src[3 * q * cols];
                lo = fminf(lo, src[(3 * q + 1) * cols]);
                hi = fmaxf(hi, src[(3 * q + 2) * cols]);
            }
        } else {
#pragma unroll 8
            for (int q = 0; q < n_parts; ++q) acc += src[3 * q * cols];
        }
        const float mu = acc / seqlen;
        mean[b * m_bs + h * m_hs + d] = mu;
        m = umax(__float_as_uint(hi - mu) & 0x7fffffffu, __float_as_uint(mu - lo) & 0x7fffffffu);
    }
    if (amax == nullptr) return;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) m = umax(m, static_cast<unsigned>(__shfl_xor(static_cast<int>(m), s, 64)));
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0)
        amax[b * a_bs + h * a_hs] = __uint_as_float(umax(umax(wave_max[0], wave_max[1]), umax(wave_max[2], wave_max[3])));
}

// 8 elements of a row: load, add the shift of the row's kv head, zero when the row is empty, round and store
template <int DT_O, int DT_OUT>
__device__ __forceinline__ void unshift_chunk(const AttnUnshiftParams& p, int b, int s, int h, int ch, bool empty) {
    float v[8];
    PrepLoad<DT_O>::to_float(PrepLoad<DT_O>::load(p.o, b * p.o_bs + s * p.o_rs + h * p.o_hs + ch * 8), v);
    if (p.shift != nullptr) {
        float c[8];
        load_f32x8(p.shift + b * p.sh_bs + (h / p.heads_per_vec) * p.sh_hs + ch * 8, c);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += c[j];
    }
    if (empty) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = 0.f;
    }
    PrepStore<DT_OUT>::store8(p.out, b * p.out_bs + s * p.out_rs + h * p.out_hs + ch * 8, v);
}

// Without lse: one thread = 8 consecutive d of one (b, s, h) row, grid stride over the rows in memory order.
template <int DT_O, int DT_OUT>
__global__ void __launch_bounds__(256) la_attn_unshift_kernel(const AttnUnshiftParams p) {
    const int chunks = p.head_dim / 8;
    const int64_t total = static_cast<int64_t>(p.batch) * p.seqlen * p.num_heads * chunks;
    for (int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; idx < total;
         idx += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int ch = static_cast<int>(idx % chunks);
        const int64_t row = idx / chunks;      // (b * S + s) * H + h
        const int h = static_cast<int>(row % p.num_heads);
        const int64_t bs = row / p.num_heads;
        unshift_chunk<DT_O, DT_OUT>(p, static_cast<int>(bs / p.seqlen), static_cast<int>(bs % p.seqlen), h, ch, false);
    }
}

// With lse: o is (b, s, h, d) and lse (b, h, s), so the flat map above would read 4 bytes of a different cache line per head. A
// workgroup takes a TILE of kUnshiftRows consecutive s x kUnshiftHeads consecutive heads of one batch instead: it reads the tile of
// lse along s (whole lines), keeps it in LDS, writes lse_out = fmaf(scale, lse_dot, lse) the same way - each element is read and
// written by ONE thread, so lse_out may be lse - and then walks the tile's chunks in the memory order of o (per s a contiguous run of
// kUnshiftHeads heads), taking the empty-row flag from LDS. Tiles by grid stride.
constexpr int kUnshiftRows = 32, kUnshiftHeads = 8;
template <int DT_O, int DT_OUT>
__global__ void __launch_bounds__(256) la_attn_unshift_lse_kernel(const AttnUnshiftParams p) {
    __shared__ float lse_tile[kUnshiftHeads * kUnshiftRows];
    const int chunks = p.head_dim / 8;
    const int s_tiles = (p.seqlen + kUnshiftRows - 1) / kUnshiftRows, h_tiles = (p.num_heads + kUnshiftHeads - 1) / kUnshiftHeads;
    const int64_t tiles = static_cast<int64_t>(p.batch) * s_tiles * h_tiles;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int ht = static_cast<int>(t % h_tiles);
        const int64_t bt = t / h_tiles;
        const int st = static_cast<int>(bt % s_tiles), b = static_cast<int>(bt / s_tiles);
        const int s0 = st * kUnshiftRows, h0 = ht * kUnshiftHeads;
        const int ns = p.seqlen - s0 < kUnshiftRows ? p.seqlen - s0 : kUnshiftRows;
        const int nh = p.num_heads - h0 < kUnshiftHeads ? p.num_heads - h0 : kUnshiftHeads;
        {
            const int hh = threadIdx.x / kUnshiftRows, ss = threadIdx.x % kUnshiftRows;      // 256 threads = 8 heads x 32 rows
            if (hh < nh && ss < ns) {
                const int64_t idx = (static_cast<int64_t>(b) * p.num_heads + h0 + hh) * p.seqlen + s0 + ss;
                const float l = p.lse[idx];
                lse_tile[threadIdx.x] = l;
                if (p.lse_out != nullptr)                              // an empty row keeps its lse; a NaN takes the normal path
                    p.lse_out[idx] = (l == INFINITY || l == -INFINITY) ? l : fmaf(p.softmax_scale, p.lse_dot[idx], l);
            }
        }
        __syncthreads();
        const int per_row = nh * chunks, items = ns * per_row;
        for (int i = threadIdx.x; i < items; i += 256) {
            const int ss = i / per_row, rest = i - ss * per_row, hh = rest / chunks, ch = rest - hh * chunks;
            const float l = lse_tile[hh * kUnshiftRows + ss];
            unshift_chunk<DT_O, DT_OUT>(p, b, s0 + ss, h0 + hh, ch, l == INFINITY || l == -INFINITY);
        }
        __syncthreads();                                               // the tile is free for the next one
    }
}

template <int DT_O, int DT_OUT>
void launch_unshift_typed(const AttnUnshiftParams& p, hipStream_t stream) {
    if (p.lse != nullptr) {
        const int64_t tiles = static_cast<int64_t>(p.batch) * ((p.seqlen + kUnshiftRows - 1) / kUnshiftRows) *
                              ((p.num_heads + kUnshiftHeads - 1) / kUnshiftHeads);
        const unsigned grid = static_cast<unsigned>(tiles < kUnshiftMaxTiles ? tiles : kUnshiftMaxTiles);
        hipLaunchKernelGGL((la_attn_unshift_lse_kernel<DT_O, DT_OUT>), dim3(grid), dim3(256), 0, stream, p);
    } else {
        const int64_t blocks = (static_cast<int64_t>(p.batch) * p.seqlen * p.num_heads * (p.head_dim / 8) + 255) / 256;
        const unsigned grid = static_cast<unsigned>(blocks < kUnshiftMaxGrid ? blocks : kUnshiftMaxGrid);
        hipLaunchKernelGGL((la_attn_unshift_kernel<DT_O, DT_OUT>), dim3(grid), dim3(256), 0, stream, p);
    }
}

// la_attn_unshift_fp8: the same restoring arithmetic, then a row-scaled e4m3 store. A UNIT is one (token, scale group): n = heads_per_scale
// * head_dim / 8 chunks, contiguous along the row when the heads are. A TEAM of `team` lanes (a power of two, at most a wave, fixed by
// the shape: unit_team) owns a unit: lane l takes chunks l, l + team, ... - C slots, C the template's bound -, loads them all
// before it converts the first, keeps them in registers as loaded (4 registers a chunk), reduces max |y| over the team by the xor
// butterfly of the bit patterns (order free), makes descale and its reciprocal once, makes y again and stores 8 bytes a chunk. No LDS
// in the reduction, no barrier, no atomics.
// A workgroup takes kAttnOutFp8Rows consecutive rows of one batch and every head: the empty-row flags of the tile come from lse in
// whole 128-byte lines along s (a byte per (head, row) in LDS; lse_out written on the way, as la_attn_unshift_lse_kernel does), then
// its teams walk the tile's units in memory order. Static mode (descale_in): no reduction, the reciprocal of the batch; the running
// maximum of the workgroup goes through four words of LDS into ONE atomicMax on the bit pattern.
// STAGE: the batch's shift rows lie in LDS behind the flags (the launcher decides: a shift that fits). A unit reads its shift twice,
// 32 bytes for every 16 of o, chunk after chunk: from LDS that is a short wait each, from the L2 a trip each.
template <int DT_O, int C, bool STAGE>
__global__ void __launch_bounds__(256) la_attn_out_fp8_kernel(const AttnUnshiftParams p, const int team) {
    extern __shared__ __attribute__((aligned(16))) unsigned char empty_tile[];     // [num_heads][kAttnOutFp8Rows] flags (read only with lse)
    __shared__ unsigned wave_max[4];
    float* const shift_tile = reinterpret_cast<float*>(empty_tile + p.num_heads * kAttnOutFp8Rows);     // [H / heads_per_vec][D]
    const int cph = p.head_dim / 8, n = p.heads_per_scale * cph, groups = p.num_heads / p.heads_per_scale;
    const int s_tiles = (p.seqlen + kAttnOutFp8Rows - 1) / kAttnOutFp8Rows;
    const int b = static_cast<int>(blockIdx.x / s_tiles), s0 = static_cast<int>(blockIdx.x % s_tiles) * kAttnOutFp8Rows;
    const int ns = p.seqlen - s0 < kAttnOutFp8Rows ? p.seqlen - s0 : kAttnOutFp8Rows;
    if (p.lse != nullptr) {
        for (int i = threadIdx.x; i < p.num_heads * kAttnOutFp8Rows; i += 256) {
            const int hh = i / kAttnOutFp8Rows, ss = i % kAttnOutFp8Rows;
            if (ss < ns) {
                const int64_t idx = (static_cast<int64_t>(b) * p.num_heads + hh) * p.seqlen + s0 + ss;
                const float l = p.lse[idx];
                const bool empty = l == INFINITY || l == -INFINITY;    // a NaN takes the normal path
                empty_tile[i] = empty;
                if (p.lse_out != nullptr) p.lse_out[idx] = empty ? l : fmaf(p.softmax_scale, p.lse_dot[idx], l);
            }
        }
    }
    if constexpr (STAGE) {
        const int per_head = p.head_dim / 4;
        for (int i = threadIdx.x; i < (p.num_heads / p.heads_per_vec) * per_head; i += 256) {
            const int hv = i / per_head, d4 = i - hv * per_head;
            reinterpret_cast<pq_f32x4*>(shift_tile)[i] = *reinterpret_cast<const pq_f32x4*>(p.shift + b * p.sh_bs + hv * p.sh_hs + d4 * 4);
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & (team - 1), teams = 256 / team;
    // (head of the group, chunk of the head) of the lane's first chunk, and the step from one of its chunks to the next
    const int hh0 = lane / cph, ch0 = lane - hh0 * cph, dh = team / cph, dc = team - dh * cph;
    const float inv_static = p.descale_in != nullptr ? __fdiv_rn(1.f, p.descale_in[b * p.di_bs]) : 0.f;
    unsigned run_max = 0;
    for (int u = threadIdx.x / team; u < ns * groups; u += teams) {
        const int ss = u / groups, g = u - ss * groups, s = s0 + ss;
        const int64_t o_row = b * p.o_bs + s * p.o_rs, out_row = b * p.out_bs + s * p.out_rs;
        typename PrepLoad<DT_O>::raw w[C];
        {
            int hh = hh0, ch = ch0;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                w[c] = lane + c * team < n ? PrepLoad<DT_O>::load(p.o, o_row + (g * p.heads_per_scale + hh) * p.o_hs + ch * 8)
                                           : PrepLoad<DT_O>::zero();
                hh += dh; ch += dc;
                if (ch >= cph) { ch -= cph; ++hh; }
            }
        }
        // y of the lane's chunk c: the restoring arithmetic of unshift_chunk. Made twice - for the maximum, then for the store - from
        // the same registers, shift and flags by the same operations (the same bits): a lane keeps 4 registers a chunk, not 8
        const auto restore = [&](int c, int hh, int ch, float (&y)[8]) {
            const int h = g * p.heads_per_scale + hh;
            PrepLoad<DT_O>::to_float(w[c], y);
            if (STAGE || p.shift != nullptr) {
                float sh[8];
                if constexpr (STAGE) load_f32x8(shift_tile + (h / p.heads_per_vec) * p.head_dim + ch * 8, sh);
                else load_f32x8(p.shift + b * p.sh_bs + (h / p.heads_per_vec) * p.sh_hs + ch * 8, sh);
#pragma unroll
                for (int j = 0; j < 8; ++j) y[j] += sh[j];
            }
            if (p.lse != nullptr && empty_tile[h * kAttnOutFp8Rows + ss]) {
#pragma unroll
                for (int j = 0; j < 8; ++j) y[j] = 0.f;
            }
        };
        float inv = inv_static;
        if (p.descale_in == nullptr || p.amax != nullptr) {
            unsigned m = 0;
            int hh = hh0, ch = ch0;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                if (lane + c * team < n) {
                    float y[8];
                    restore(c, hh, ch, y);
                    m = umax(m, absmax8(y));
                }
                hh += dh; ch += dc;
                if (ch >= cph) { ch -= cph; ++hh; }
            }
            if (p.descale_in == nullptr) {
#pragma unroll
                for (int sft = 32; sft >= 1; sft >>= 1)
                    if (sft < team) m = umax(m, static_cast<unsigned>(__shfl_xor(static_cast<int>(m), sft, 64)));
                const float amax = __uint_as_float(m);                 // a NaN fails the compare and stays
                const float descale = __fdiv_rn(amax < 0x1p-100f ? 0x1p-100f : amax, 448.f);
                inv = __fdiv_rn(1.f, descale);
                if (lane == 0) p.row_descale[b * p.rd_bs + s * p.rd_rs + g * p.rd_gs] = descale;
            } else {
                run_max = umax(run_max, m);
            }
        }
        {
            int hh = hh0, ch = ch0;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                if (lane + c * team < n) {
                    float y[8];
                    restore(c, hh, ch, y);
                    scale_clamp8(y, inv);
                    PrepStore<2>::store8(p.out, out_row + (g * p.heads_per_scale + hh) * p.out_hs + ch * 8, y);
                }
                hh += dh; ch += dc;
                if (ch >= cph) { ch -= cph; ++hh; }
            }
        }
    }
    if (p.descale_in != nullptr && p.amax != nullptr) {
#pragma unroll
        for (int sft = 32; sft >= 1; sft >>= 1) run_max = umax(run_max, static_cast<unsigned>(__shfl_xor(static_cast<int>(run_max), sft, 64)));
        if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = run_max;
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned wg = umax(umax(wave_max[0], wave_max[1]), umax(wave_max[2], wave_max[3]));
            if (wg) atomicMax(reinterpret_cast<unsigned*>(p.amax + b * p.am_bs), wg);
        }
    }
}

// lanes of a team for n chunks a unit: the next power of two, at most a wave. A function of the shape alone.
inline int unit_team(int n) {
    int t = 1;
    while (t < n && t < 64) t <<= 1;
    return t;
}

constexpr size_t kAttnOutFp8MaxLds = 64 * 1024;      // dynamic LDS a launch may ask for without opting in to more

template <int DT_O, bool STAGE>
void launch_out_fp8_staged(const AttnUnshiftParams& p, size_t lds, hipStream_t stream) {
    const int n = p.heads_per_scale * (p.head_dim / 8), team = unit_team(n), per_lane = (n + team - 1) / team;      // <= 32: la_api.hip
    const dim3 grid(static_cast<unsigned>(static_cast<int64_t>(p.batch) * ((p.seqlen + kAttnOutFp8Rows - 1) / kAttnOutFp8Rows)));
    if (per_lane <= 1) hipLaunchKernelGGL((la_attn_out_fp8_kernel<DT_O, 1, STAGE>), grid, dim3(256), lds, stream, p, team);
    else if (per_lane <= 4) hipLaunchKernelGGL((la_attn_out_fp8_kernel<DT_O, 4, STAGE>), grid, dim3(256), lds, stream, p, team);
    else if (per_lane <= 10) hipLaunchKernelGGL((la_attn_out_fp8_kernel<DT_O, 10, STAGE>), grid, dim3(256), lds, stream, p, team);
    else if (per_lane <= 16) hipLaunchKernelGGL((la_attn_out_fp8_kernel<DT_O, 16, STAGE>), grid, dim3(256), lds, stream, p, team);
    else hipLaunchKernelGGL((la_attn_out_fp8_kernel<DT_O, 32, STAGE>), grid, dim3(256), lds, stream, p, team);
}

template <int DT_O>
void launch_out_fp8(const AttnUnshiftParams& p, hipStream_t stream) {
    const size_t flags = static_cast<size_t>(p.num_heads) * kAttnOutFp8Rows;      // a multiple of 16 bytes: the shift rows behind it are aligned
    const size_t rows = p.shift != nullptr ? static_cast<size_t>(p.num_heads / p.heads_per_vec) * p.head_dim * sizeof(float) : 0;
    if (rows != 0 && flags + rows <= kAttnOutFp8MaxLds) launch_out_fp8_staged<DT_O, true>(p, flags + rows, stream);
    else launch_out_fp8_staged<DT_O, false>(p, flags, stream);
}

template <int DT_O>
void launch_unshift_o(const AttnUnshiftParams& p, int out_dtype, hipStream_t stream) {
    if (out_dtype == 0) launch_unshift_typed<DT_O, 0>(p, stream);
    else if (out_dtype == 1) launch_unshift_typed<DT_O, 1>(p, stream);
    else if (out_dtype == 2) launch_out_fp8<DT_O>(p, stream);
    else launch_unshift_typed<DT_O, 3>(p, stream);
}

}  // namespace

hipError_t launch_v_colstats(const VColstatsParams& p, int in_dtype, hipStream_t stream) {
    (void)hipGetLastError();
    const int64_t items = static_cast<int64_t>(p.n_parts) * p.batch * p.num_heads * (p.head_dim / 8);
    const dim3 grid(static_cast<unsigned>((items + 255) / 256)), block(256);
    if (in_dtype == 0) hipLaunchKernelGGL(la_v_colstats_kernel<0>, grid, block, 0, stream, p);
    else if (in_dtype == 1) hipLaunchKernelGGL(la_v_colstats_kernel<1>, grid, block, 0, stream, p);
    else hipLaunchKernelGGL(la_v_colstats_kernel<3>, grid, block, 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_v_colstats_finish(const float* part, int n_parts, int batch, int num_heads, int head_dim, int seqlen, float* mean,
                                    int64_t m_bs, int64_t m_hs, float* amax, int64_t a_bs, int64_t a_hs, hipStream_t stream) {
    (void)hipGetLastError();
    const int64_t cols = static_cast<int64_t>(batch) * num_heads * head_dim;
    hipLaunchKernelGGL(la_v_colstats_finish_kernel, dim3(static_cast<unsigned>(batch) * static_cast<unsigned>(num_heads)), dim3(256), 0,
                       stream, part, n_parts, cols, head_dim, num_heads, static_cast<float>(seqlen), mean, m_bs, m_hs, amax, a_bs, a_hs);
    return hipGetLastError();
}

hipError_t launch_attn_unshift(const AttnUnshiftParams& p, int o_dtype, int out_dtype, hipStream_t stream) {
    (void)hipGetLastError();
    if (o_dtype == 0) launch_unshift_o<0>(p, out_dtype, stream);
    else launch_unshift_o<1>(p, out_dtype, stream);
    return hipGetLastError();
}

}  // namespace la
