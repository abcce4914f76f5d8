// la_prep_qk.hip — the q / k prologue of a Wan2.x-style attention block in ONE pass (la_qk_prep): RMSNorm over the token (or over each
// head, or none), 3-axis RoPE on interleaved pairs from host-built (cos, sin) tables, the cast to bf16 / fp16. x is read once and out is
// written once; between the two everything is fp32 and the only rounding is the one at the store.
//
// Mapping: one WAVE per token (b, s), four tokens per 256-thread workgroup (tokens above 5120 elements under LA_NORM_TOKEN: one
// workgroup per token), grid-stride over tokens with at most kMaxGrid workgroups.
// The token is cut into chunks of 8 consecutive elements (one 16-byte load of 16-bit elements, two of fp32; one 16-byte store); a chunk
// never straddles a head (head_dim % 8 == 0). What a lane needs that does not depend on the token - the column and the offsets of its
// chunks, the axis and table column of the rotation pairs it stages - is resolved before the token loop; its slice of the weight is the
// same for every token and is reread from L1 / L2 (keeping it in registers too costs the occupancy the stream needs).
//
//  * la_qk_prep_token_kernel<IN, OUT, NCH, WG> (LA_NORM_TOKEN): lane l owns chunks l, l + 64, ... (NCH <= 10 of them, NCH * 512 >=
//    H * D), keeps all of them in registers from the load to the store, sums its squares chunk by chunk (a fixed pairwise tree inside
//    a chunk), and the wave finishes the sum with a 6-step xor butterfly: the order of every addition depends on the shape alone,
//    every lane holds the same bits, two launches agree bitwise. No atomics, no workspace. Above H * D = 5120 (WG) the four waves of
//    the workgroup share ONE token (chunks tid, tid + 256, ..., at most 8 per lane: H * D <= 16384, the limit la_qk_prep states) and
//    their four sums are added in a fixed order through LDS: 32 chunks per lane of one wave do not fit the register file.
//  * la_qk_prep_head_kernel<IN, OUT> (LA_NORM_HEAD, LA_NORM_NONE): a head's D / 8 chunks sit on G = 2^ceil(log2(D / 8)) <= 32
//    neighbouring lanes (lanes past D / 8 idle), 64 / G heads per pass, kHeadUnroll passes loaded together; the sum of a head is the
//    xor butterfly over its G lanes.
//
// The rotation of a token is one row of at most head_dim / 2 (cos, sin) pairs - row c_a of table a for the pairs axis a owns, (1, 0)
// behind them - the same for every head. The wave gathers it into its own 1 KiB of LDS once per token (two pairs per lane, 8-byte
// loads that hit L2: the three tables together are (e0 + e1 + e2) * D / 2 * 8 bytes) and every chunk reads its four pairs from there
// with two 16-byte LDS loads: the axis of a pair is looked up per PAIR while staging, never per chunk (at head_dim 128 the axis
// boundaries fall at elements 44 and 86, inside a chunk). Only the wave that wrote a row reads it: LDS instructions of one wave execute
// in order, a wavefront-scope fence keeps the compiler from reordering them, no workgroup barrier is needed and waves of a workgroup
// may run different numbers of tokens.
//
// In-place (out == x with equal strides and element sizes): a chunk is stored by the lane that loaded it, after every load of its
// token (token kernel) or of its batch of passes (head kernel); x and out carry no __restrict__.
//
// Arithmetic: r = rsqrt(sum(x^2) / n + eps) with the sum in fp32 as in the torch expression it replaces (a token whose squares
// overflow fp32 gives r = 0 there and here); y = (x * r) * w; out = (y0 cos - y1 sin, y0 sin + y1 cos). One fewer rounding than Wan's
// `.type_as(x) * weight` followed by a rope that rounds again: DESIGN.md §7.
//
// The e4m3 output form (la_qk_prep_fp8; PrepPolicy<1>: quantize, PrepPolicy<2>: the amax pass alone, nothing stored). y above is
// computed by the same instructions in the same order; two steps follow it:
//  * amax: the unsigned maximum over the bit patterns of |y| (order-free; any NaN wins), per lane in registers (token kernel) or per
//    head over its G lanes (head kernel), then per head in LDS with ds atomics, and ONE global atomicMax per (scale group, batch) when
//    the workgroup leaves a batch. For that the workgroup must leave a batch as a whole: the loop of these forms runs over ROUNDS of
//    4 consecutive tokens of ONE batch (one token when the workgroup shares it), the same trips for every thread, batches in rising
//    order; a round past the end of its batch keeps its spare waves idle (they load, stage and store nothing).
//  * quantize: z = y * inv, inv = 1 / descale one IEEE division per group when the workgroup enters a batch (kept per head in LDS);
//    z is clamped to +-448 by two compares that a NaN fails, so a NaN stays a NaN; then the hardware's round-to-nearest-even e4m3
//    conversion (OCP e4m3fn on gfx950) of values that cannot overflow: no mode bit matters. 8 elements = 8 bytes, one 8-byte store.
//
// K smoothing (la_qk_prep_smooth; PrepPolicy<3>, and PrepPolicy<4> when nothing is stored; the same two templates). y is computed as
// above; then, each step on when its pointer is given: the column sums and the row dots take y, y' = y - shift[b][h][:] (one fp32
// subtraction), and amax / quantize take y'.
//  * rows -> workgroups: a batch's rows are cut into PARTS of part_rows consecutive rows (qk_prep_part_rows: a function of the sequence
//    length alone), a workgroup takes a BLOCK of 4 parts of one batch, one part per wave (when the workgroup shares a token: the 4
//    parts one after the other), blocks by grid stride. Every thread runs the same trips, so the barriers of scale_turn still meet.
//  * column sums: a thread's running sums of ITS columns live in LDS (colsum_lds, dynamic: 8 KiB per chunk slot, only when asked for)
//    - no register is spent on them and no other thread touches them, so there is no atomic and no barrier. They start at 0 with a
//    part's first row, take the rows in order and go to part[p][b][h][d] behind its last row with two 16-byte vector stores per chunk:
//    the bits depend on (S, H, D) alone. la_colsum_finish_kernel adds the parts in index order and divides by S.
//  * row dots: a chunk's share (a fixed tree of its 8 products) goes to LDS by chunk index; one thread per head adds the D / 8 shares
//    in column order (token kernel), or the head's G lanes run the xor butterfly (head kernel). One 4-byte vector store per (head, row).
//
// Row maps (the _rows entry points; every form of both templates): out row s is made from row src_rows[s] of x and rotated as position
// pos_offset + positions[s] (map_row; NULL tables: s and the source row). The wave that owns a token reads its two table entries, one
// 4-byte load each, in front of the token's loads; everything behind the load - sums, rotation, maxima, column parts, row dots, the
// store - is indexed by the OUT row and unchanged. Without tables the two values are s and pos_offset + s: the bits of an unmapped launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "la_kernel_params.h"
#include "la_prep_common.h"

namespace la {
namespace {

constexpr int kMaxGrid = 2048;             // workgroups: 8 per compute unit; the rest of the tokens by grid stride
constexpr int kRotRow = 128;               // pairs of one token's rotation row (head_dim <= 256)
constexpr int kHeadUnroll = 4;             // passes of the head kernel whose loads are issued together

// What follows y: 0 the 16-bit store of la_qk_prep; 1 amax + scale + clamp + e4m3 store; 2 amax alone (x is read, nothing is written);
// 3 / 4 la_qk_prep_smooth: 1 / 2 of y - shift, plus the column sums and row dots of y (each on when its pointer is given)
template <int MODE> struct PrepPolicy {
    static constexpr bool kScaled = MODE != 0;                     // per-head LDS tables, the loop over rounds
    static constexpr bool kStore = MODE == 0 || MODE == 1 || MODE == 3;
    static constexpr bool kSmooth = MODE >= 3;                     // the loop over blocks of 4 parts, each part's rows in order
};

// The running column sums of la_qk_prep_smooth: element j of chunk slot q of thread t at ((q * 8 + j) * 256 + t). A thread reads and
// writes its own words only: no barrier, no atomic, and the order of the additions is the order of the rows.
extern __shared__ float colsum_lds[];

__device__ __forceinline__ void colsum_zero(int slots) {
    for (int q = 0; q < slots * 8; ++q) colsum_lds[q * 256 + threadIdx.x] = 0.f;
}
__device__ __forceinline__ void colsum_add8(int slot, const float (&y)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) colsum_lds[(slot * 8 + j) * 256 + threadIdx.x] += y[j];
}
__device__ __forceinline__ void colsum_flush8(int slot, float* dst) {
    float* t = colsum_lds + slot * 8 * 256 + threadIdx.x;
    *reinterpret_cast<pq_f32x4*>(dst) = pq_f32x4{t[0], t[256], t[512], t[768]};
    *reinterpret_cast<pq_f32x4*>(dst + 4) = pq_f32x4{t[1024], t[1280], t[1536], t[1792]};
}

__device__ __forceinline__ float dot8(const float (&y)[8], const float (&c)[8]) {
    return ((y[0] * c[0] + y[1] * c[1]) + (y[2] * c[2] + y[3] * c[3])) + ((y[4] * c[4] + y[5] * c[5]) + (y[6] * c[6] + y[7] * c[7]));
}

// The workgroup leaves batch old_b (-1: none) and enters new_b (-1: none): the maxima its waves collected per head in am_tab go out,
// one atomic per scale group, and the reciprocal scales of new_b come in. Every thread of the workgroup calls it at the same trip.
template <bool STORE>
__device__ __forceinline__ void scale_turn(const QkPrepParams& p, unsigned* am_tab, float* inv_tab, int64_t old_b, int64_t new_b) {
    __syncthreads();                                               // am_tab is complete, inv_tab no longer read
    const int hps = p.heads_per_scale, groups = p.num_heads / hps;
    for (int g = threadIdx.x; g < groups; g += 256) {
        unsigned m = 0;
        for (int j = 0; j < hps; ++j) {
            m = umax(m, am_tab[g * hps + j]);
            am_tab[g * hps + j] = 0;
        }
        if (old_b >= 0 && p.amax && m) atomicMax(reinterpret_cast<unsigned*>(p.amax + old_b * p.am_bs + g * p.am_hs), m);
        if (STORE && new_b >= 0) {
            const float inv = p.descale ? __fdiv_rn(1.f, p.descale[new_b * p.ds_bs + g * p.ds_hs]) : 1.f;
            for (int j = 0; j < hps; ++j) inv_tab[g * hps + j] = inv;
        }
    }
    __syncthreads();
}

__device__ __forceinline__ float sum_squares8(const float (&v)[8]) {
    return ((v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3])) + ((v[4] * v[4] + v[5] * v[5]) + (v[6] * v[6] + v[7] * v[7]));
}

// LDS accesses of ONE wave before / after this point stay on their side of it (the hardware runs them in order)
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The two rotation pairs a lane stages per token (pairs lane and lane + 64 of the row): axis (-1: behind the rotated pairs) and column
// inside the axis' table row. Token independent.
struct RotStage {
    int axis[2], col[2];
    __device__ __forceinline__ void init(const QkPrepParams& p, int lane) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int j = lane + 64 * k, p1 = p.pairs[0], p2 = p.pairs[0] + p.pairs[1], p3 = p2 + p.pairs[2];
            axis[k] = j >= p3 ? -1 : (j >= p1) + (j >= p2);
            col[k] = j - (j >= p2 ? p2 : (j >= p1 ? p1 : 0));
        }
    }
    // gather the row of position `pos` (wave-uniform) into `row` (this wave's kRotRow pairs of LDS)
    __device__ __forceinline__ void stage(const QkPrepParams& p, int pos, int lane, float* row) const {
        const int plane = p.ext1 * p.ext2;
        const int c0 = pos / plane, rem = pos - c0 * plane, c1 = rem / p.ext2, c2 = rem - c1 * p.ext2;
        const float* __restrict__ r0 = p.table[0] + static_cast<int64_t>(c0) * p.pairs[0] * 2;
        const float* __restrict__ r1 = p.table[1] + static_cast<int64_t>(c1) * p.pairs[1] * 2;
        const float* __restrict__ r2 = p.table[2] + static_cast<int64_t>(c2) * p.pairs[2] * 2;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            pq_f32x2 cs = {1.f, 0.f};
            if (axis[k] >= 0) cs = *reinterpret_cast<const pq_f32x2*>((axis[k] == 0 ? r0 : (axis[k] == 1 ? r1 : r2)) + 2 * col[k]);
            *reinterpret_cast<pq_f32x2*>(row + 2 * (lane + 64 * k)) = cs;
        }
    }
};

// The row of x that out row s of batch b is made from and the position it is rotated as (s: wave-uniform and inside the sequence).
// Without a table: (s, pos_offset + s), what a launch without a map computes. With one (the _rows entry points) the source row is
// clamped into [0, src_seqlen) and the position into [0, pos_limit): no entry of a table can take a load outside x or the rope tables.
__device__ __forceinline__ void map_row(const QkPrepParams& p, int64_t b, int s, int& src, int& pos) {
    src = s;
    pos = p.pos_offset + s;
    if (p.src_rows || p.positions) {
        const int64_t at = b * p.map_bs + s;
        if (p.src_rows) {
            const int r = __builtin_amdgcn_readfirstlane(p.src_rows[at]);
            src = r < 0 ? 0 : (r < p.src_seqlen ? r : p.src_seqlen - 1);
        }
        const int64_t q = static_cast<int64_t>(p.pos_offset) + (p.positions ? __builtin_amdgcn_readfirstlane(p.positions[at]) : src);
        pos = static_cast<int>(q < 0 ? 0 : (q < p.pos_limit ? q : p.pos_limit - 1));
    }
}

// y (8 elements starting at element e of a head) *= scale * w, then the pairs below `rot_pairs` are rotated by the staged row
template <bool ROT>
__device__ __forceinline__ void scale_rotate8(float (&y)[8], float r, const float (&w)[8], int e, int rot_pairs, const float* row) {
#pragma unroll
    for (int i = 0; i < 8; ++i) y[i] = (y[i] * r) * w[i];
    if (ROT) {
        const pq_f32x4 t0 = *reinterpret_cast<const pq_f32x4*>(row + e), t1 = *reinterpret_cast<const pq_f32x4*>(row + e + 4);
        const float cs[8] = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float a = y[2 * k], b = y[2 * k + 1], c = cs[2 * k], s = cs[2 * k + 1];
            const bool on = (e >> 1) + k < rot_pairs;              // a pair behind the rotated ones passes through untouched (inf stays inf)
            y[2 * k] = on ? a * c - b * s : a;
            y[2 * k + 1] = on ? a * s + b * c : b;
        }
    }
}

// WG false: one wave per token. WG true (H * D > 5120): the four waves of the workgroup share one token, so that a lane still keeps
// at most 10 chunks; the four partial sums meet in LDS and are added in a fixed order.
template <int DT_IN, int DT_OUT, int NCH, bool WG, int MODE>
__global__ void __launch_bounds__(256) la_qk_prep_token_kernel(const QkPrepParams p) {
    typedef PrepPolicy<MODE> POL;
    __shared__ __attribute__((aligned(16))) float rot_lds[4][2 * kRotRow];
    __shared__ float part[4];
    __shared__ unsigned am_tab[POL::kScaled ? kQkPrepScaleSlots : 1];
    __shared__ float inv_tab[POL::kScaled ? kQkPrepScaleSlots : 1];
    __shared__ float dot_lds[POL::kSmooth ? NCH * 256 : 1];        // smooth: a chunk's share of its head's row dot, by chunk (and wave)
    typedef typename PrepLoad<DT_IN>::raw raw_t;
    constexpr int kLanes = WG ? 256 : 64;                          // lanes that share a token
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int D = p.head_dim, n = p.num_heads * D, nchunks = n >> 3;
    const int rot_pairs = p.pairs[0] + p.pairs[1] + p.pairs[2];
    const bool rotate = p.rotate != 0;
    const float* __restrict__ weight = p.weight;
    float* row = rot_lds[wave];                                    // WG: every wave stages its own copy of the token's row
    const int first = WG ? static_cast<int>(threadIdx.x) : lane;
    constexpr bool store = POL::kStore;
    float* dots = dot_lds + (WG ? 0 : wave * NCH * 64);

    // chunk i of this lane = chunk first + kLanes i of the token: its first element inside its head (-1: no such chunk) and its
    // element offsets from the token's start in x and out (below 2^31, checked by la_qk_prep)
    int col[NCH], x_off[NCH], o_off[NCH];
    unsigned am[NCH];                                              // e4m3 forms: this lane's running maxima of the current batch, per chunk
    // ... and the head of chunk i, recomputed where it is needed (a register per chunk costs the e4m3 forms a wave of occupancy):
    // floor((c8 + 0.5) / D) in fp32 is exact for c8 < 16384, D <= 256 (the quotient stays 0.5 / 256 away from an integer)
    const float rcp_d = 1.f / static_cast<float>(D);
    const auto head_of = [&](int i) { return static_cast<int>((static_cast<float>((first + kLanes * i) * 8) + 0.5f) * rcp_d); };
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = first + kLanes * i;
        const int head = (c * 8) / D;
        am[i] = 0;
        col[i] = c < nchunks ? c * 8 - head * D : -1;
        x_off[i] = static_cast<int>(head * p.x_hs) + col[i];
        o_off[i] = static_cast<int>(head * p.o_hs) + col[i];
    }
    RotStage rs;
    rs.init(p, lane);

    const int64_t t0 = WG ? static_cast<int64_t>(blockIdx.x) : static_cast<int64_t>(blockIdx.x) * 4 + wave;
    const int64_t t_step = WG ? static_cast<int64_t>(gridDim.x) : static_cast<int64_t>(gridDim.x) * 4;
    // e4m3 forms: t counts rounds (kPerRound consecutive tokens of one batch), the same trips for every thread
    constexpr int kPerRound = WG ? 1 : 4;
    const int64_t rpb = (p.seqlen + kPerRound - 1) / kPerRound;
    // smooth: t counts blocks of 4 parts of one batch; a wave walks the rows of its part in order (WG: the workgroup walks the 4 parts
    // one after the other), `trips` rounds, the same for every thread
    const int part_rows = POL::kSmooth ? p.part_rows : 1, trips = POL::kSmooth ? (WG ? 4 * part_rows : part_rows) : 1;
    const int64_t t_end = POL::kSmooth ? static_cast<int64_t>(p.batch) * p.part_blocks : (POL::kScaled ? p.tokens / p.seqlen * rpb : p.tokens);
    int64_t cur_b = -1;
    if (POL::kScaled)
        for (int h = threadIdx.x; h < p.num_heads; h += 256) am_tab[h] = 0;      // (the first scale_turn starts with a barrier)
    for (int64_t t = POL::kScaled ? static_cast<int64_t>(blockIdx.x) : t0; t < t_end; t += POL::kScaled ? static_cast<int64_t>(gridDim.x) : t_step)
    for (int trip = 0; trip < trips; ++trip) {
        int64_t b;                                                 // WG: the same trips for every thread of the workgroup
        int s;
        bool live = true;                                          // false: a spare wave of a batch's last round
        int part_row = 0;                                          // smooth: the row inside its part, and the part
        int64_t part_id = 0;
        if constexpr (POL::kScaled) {
            if constexpr (POL::kSmooth) {
                b = t / p.part_blocks;
                const int sub = WG ? trip / part_rows : wave;
                part_row = WG ? trip - sub * part_rows : trip;
                part_id = (t - b * p.part_blocks) * 4 + sub;
                const int64_t s64 = part_id * part_rows + part_row;
                live = s64 < p.seqlen;
                s = static_cast<int>(live ? s64 : 0);
                if (p.colsum_part && part_row == 0) colsum_zero(NCH);
            } else {
                b = t / rpb;
                s = static_cast<int>(t - b * rpb) * kPerRound + (WG ? 0 : wave);
                live = s < p.seqlen;
            }
            if (b != cur_b) {
#pragma unroll
                for (int i = 0; i < NCH; ++i) {
                    if (col[i] >= 0 && am[i]) atomicMax(&am_tab[head_of(i)], am[i]);
                    am[i] = 0;
                }
                scale_turn<POL::kStore>(p, am_tab, inv_tab, cur_b, b);
                cur_b = b;
            }
        } else {
            b = t / p.seqlen;
            s = static_cast<int>(t - b * p.seqlen);
        }
        int src, pos;                                              // x is read at row src, everything else speaks of the out row s
        map_row(p, b, live ? s : 0, src, pos);
        const int64_t x_tok = b * p.x_bs + src * p.x_rs, o_tok = b * p.o_bs + s * p.o_rs;
        raw_t v[NCH];                                              // the token: it stays in registers until it is stored
#pragma unroll
        for (int i = 0; i < NCH; ++i) v[i] = col[i] >= 0 && live ? PrepLoad<DT_IN>::load(p.x, x_tok + x_off[i]) : PrepLoad<DT_IN>::zero();
        if (rotate && live) rs.stage(p, pos, lane, row);
        float ss = 0.f;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            float y[8];
            PrepLoad<DT_IN>::to_float(v[i], y);
            ss += sum_squares8(y);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
        if (WG) {
            if (lane == 0) part[wave] = ss;
            __syncthreads();
            ss = (part[0] + part[1]) + (part[2] + part[3]);
            __syncthreads();                                       // part is rewritten for the next token
        }
        const float r = rsqrtf(ss / static_cast<float>(n) + p.eps);
        if (rotate) wave_lds_fence();
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            if (col[i] >= 0 && live) {
                float y[8], w[8];
                PrepLoad<DT_IN>::to_float(v[i], y);
#pragma unroll
                for (int j = 0; j < 8; ++j) w[j] = 1.f;
                if (weight) load_f32x8(weight + (first + kLanes * i) * 8, w);       // 4 H D bytes every token rereads: they stay in L1 / L2
                if (rotate) scale_rotate8<true>(y, r, w, col[i], rot_pairs, row);
                else scale_rotate8<false>(y, r, w, col[i], rot_pairs, row);
                if constexpr (POL::kSmooth) {                      // sums and dots see y, the maximum and the store y - shift
                    if (p.colsum_part) colsum_add8(i, y);
                    if (p.dot_vec) {
                        float c[8];
                        load_f32x8(p.dot_vec + b * p.dv_bs + (head_of(i) / p.heads_per_dot) * p.dv_hs + col[i], c);
                        dots[first + kLanes * i] = dot8(y, c);
                    }
                    if (p.shift) {
                        float c[8];
                        load_f32x8(p.shift + b * p.sh_bs + head_of(i) * p.sh_hs + col[i], c);
#pragma unroll
                        for (int j = 0; j < 8; ++j) y[j] -= c[j];
                    }
                }
                if constexpr (POL::kScaled) {
                    am[i] = umax(am[i], absmax8(y));
                    if (store) scale_clamp8(y, inv_tab[head_of(i)]);
                }
                if (store) PrepStore<DT_OUT>::store8(p.out, o_tok + o_off[i], y);
            }
        }
        if constexpr (POL::kSmooth) {
            if (p.dot_vec) {                                       // a head's D / 8 shares, added in column order by one thread
                if (WG) __syncthreads();                           // (the next token writes `dots` behind its own barriers)
                else wave_lds_fence();
                const int cph = D >> 3;
                for (int h = first; h < p.num_heads && live; h += kLanes) {
                    float acc = 0.f;
                    for (int k = 0; k < cph; ++k) acc += dots[h * cph + k];
                    p.dot_out[(b * p.num_heads + h) * p.seqlen + s] = acc;
                }
                if (!WG) wave_lds_fence();
            }
            if (p.colsum_part && part_row == part_rows - 1) {
                float* dst = p.colsum_part + (part_id * p.batch + b) * n;
#pragma unroll
                for (int i = 0; i < NCH; ++i)
                    if (col[i] >= 0) colsum_flush8(i, dst + (first + kLanes * i) * 8);
            }
        }
        if (rotate) wave_lds_fence();                              // the next token's row is staged behind this token's reads
    }
    if constexpr (POL::kScaled) {
#pragma unroll
        for (int i = 0; i < NCH; ++i)
            if (col[i] >= 0 && am[i]) atomicMax(&am_tab[head_of(i)], am[i]);
        scale_turn<false>(p, am_tab, inv_tab, cur_b, -1);
    }
}

template <int DT_IN, int DT_OUT, int MODE>
__global__ void __launch_bounds__(256) la_qk_prep_head_kernel(const QkPrepParams p, int group_log2) {
    typedef PrepPolicy<MODE> POL;
    __shared__ __attribute__((aligned(16))) float rot_lds[4][2 * kRotRow];
    __shared__ unsigned am_tab[POL::kScaled ? kQkPrepScaleSlots : 1];
    __shared__ float inv_tab[POL::kScaled ? kQkPrepScaleSlots : 1];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int D = p.head_dim, H = p.num_heads;
    const int G = 1 << group_log2, heads_per_pass = 64 >> group_log2;
    const int sub = lane >> group_log2, e = (lane & (G - 1)) * 8;  // this lane: head `sub` of a pass, elements [e, e + 8) of it
    const bool col_ok = e < D;
    const bool norm = p.norm_mode == 2;
    const int rot_pairs = p.pairs[0] + p.pairs[1] + p.pairs[2];
    const bool rotate = p.rotate != 0;
    float* row = rot_lds[wave];
    float w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = 1.f;
    if (norm && p.weight && col_ok) load_f32x8(p.weight + e, w);
    RotStage rs;
    rs.init(p, lane);

    // e4m3 forms: t counts rounds (4 consecutive tokens of one batch), the same trips for every thread
    const int64_t rpb = (p.seqlen + 3) / 4;
    // smooth: t counts blocks of 4 parts of one batch, a wave walks the rows of its part in order; a thread's column sums: slot
    // (pass * kHeadUnroll + u) of colsum_lds
    const int trips = POL::kSmooth ? p.part_rows : 1;
    const int sum_slots = (H + heads_per_pass * kHeadUnroll - 1) / (heads_per_pass * kHeadUnroll) * kHeadUnroll;
    constexpr bool store = POL::kStore;
    const int64_t t_end = POL::kSmooth ? static_cast<int64_t>(p.batch) * p.part_blocks : (POL::kScaled ? p.tokens / p.seqlen * rpb : p.tokens);
    int64_t cur_b = -1;
    if (POL::kScaled)
        for (int h = threadIdx.x; h < H; h += 256) am_tab[h] = 0;                // (the first scale_turn starts with a barrier)
    for (int64_t t = POL::kScaled ? static_cast<int64_t>(blockIdx.x) : static_cast<int64_t>(blockIdx.x) * 4 + wave; t < t_end;
         t += POL::kScaled ? static_cast<int64_t>(gridDim.x) : static_cast<int64_t>(gridDim.x) * 4)
    for (int trip = 0; trip < trips; ++trip) {
        int64_t b;
        int s;
        bool live = true;                                          // false: a spare wave of a batch's last round
        int64_t part = 0;
        if constexpr (POL::kScaled) {
            if constexpr (POL::kSmooth) {
                b = t / p.part_blocks;
                part = (t - b * p.part_blocks) * 4 + wave;
                const int64_t s64 = part * trips + trip;
                live = s64 < p.seqlen;
                s = static_cast<int>(live ? s64 : 0);
                if (p.colsum_part && trip == 0) colsum_zero(sum_slots);
            } else {
                b = t / rpb;
                s = static_cast<int>(t - b * rpb) * 4 + wave;
                live = s < p.seqlen;
            }
            if (b != cur_b) {
                scale_turn<POL::kStore>(p, am_tab, inv_tab, cur_b, b);
                cur_b = b;
            }
        } else {
            b = t / p.seqlen;
            s = static_cast<int>(t - b * p.seqlen);
        }
        int src, pos;                                              // x is read at row src, everything else speaks of the out row s
        map_row(p, b, live ? s : 0, src, pos);
        const int64_t x_tok = b * p.x_bs + src * p.x_rs + e, o_tok = b * p.o_bs + s * p.o_rs + e;
        if (rotate) {
            if (live) rs.stage(p, pos, lane, row);
            wave_lds_fence();
        }
        for (int h0 = 0; h0 < H; h0 += heads_per_pass * kHeadUnroll) {
            typename PrepLoad<DT_IN>::raw raw[kHeadUnroll];
#pragma unroll
            for (int u = 0; u < kHeadUnroll; ++u) {
                const int h = h0 + u * heads_per_pass + sub;
                raw[u] = col_ok && h < H && live ? PrepLoad<DT_IN>::load(p.x, x_tok + h * p.x_hs) : PrepLoad<DT_IN>::zero();
            }
#pragma unroll
            for (int u = 0; u < kHeadUnroll; ++u) {
                const int h = h0 + u * heads_per_pass + sub;
                float y[8], r = 1.f;
                PrepLoad<DT_IN>::to_float(raw[u], y);
                if (norm) {                                        // uniform: every lane of the wave takes part in the butterfly
                    float ss = sum_squares8(y);
                    for (int off = G >> 1; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
                    r = rsqrtf(ss / static_cast<float>(D) + p.eps);
                }
                unsigned m = 0;
                float dot = 0.f;
                if (col_ok && h < H && live) {
                    if (rotate) scale_rotate8<true>(y, r, w, e, rot_pairs, row);
                    else scale_rotate8<false>(y, r, w, e, rot_pairs, row);
                    if constexpr (POL::kSmooth) {                  // sums and dots see y, the maximum and the store y - shift
                        if (p.colsum_part) colsum_add8(h0 / heads_per_pass + u, y);
                        if (p.dot_vec) {
                            float c[8];
                            load_f32x8(p.dot_vec + b * p.dv_bs + (h / p.heads_per_dot) * p.dv_hs + e, c);
                            dot = dot8(y, c);
                        }
                        if (p.shift) {
                            float c[8];
                            load_f32x8(p.shift + b * p.sh_bs + h * p.sh_hs + e, c);
#pragma unroll
                            for (int j = 0; j < 8; ++j) y[j] -= c[j];
                        }
                    }
                    if constexpr (POL::kScaled) {
                        m = absmax8(y);
                        if (store) scale_clamp8(y, inv_tab[h]);
                    }
                    if (store) PrepStore<DT_OUT>::store8(p.out, o_tok + h * p.o_hs, y);
                }
                if constexpr (POL::kSmooth) {
                    if (p.dot_vec) {                               // uniform: the head's dot over its G lanes, a fixed butterfly
                        for (int off = G >> 1; off > 0; off >>= 1) dot += __shfl_xor(dot, off);
                        if ((lane & (G - 1)) == 0 && h < H && live) p.dot_out[(b * H + h) * p.seqlen + s] = dot;
                    }
                }
                if constexpr (POL::kScaled) {                      // uniform: the head's maximum over its G lanes, one ds atomic per head
                    for (int off = G >> 1; off > 0; off >>= 1) m = umax(m, static_cast<unsigned>(__shfl_xor(static_cast<int>(m), off)));
                    if ((lane & (G - 1)) == 0 && m) atomicMax(&am_tab[h], m);
                }
            }
        }
        if constexpr (POL::kSmooth) {
            if (p.colsum_part && trip == trips - 1) {
                float* dst = p.colsum_part + (part * p.batch + b) * H * D + e;
                for (int q = 0; q < sum_slots; ++q) {
                    const int h = (q / kHeadUnroll) * heads_per_pass * kHeadUnroll + (q % kHeadUnroll) * heads_per_pass + sub;
                    if (col_ok && h < H) colsum_flush8(q, dst + h * D);
                }
            }
        }
        if (rotate) wave_lds_fence();
    }
    if constexpr (POL::kScaled) scale_turn<false>(p, am_tab, inv_tab, cur_b, -1);
}

// The token kernel of a shape: NCH chunks of 8 per lane, one wave per token up to 10 of them (5120 elements), above that the four waves
// of the workgroup share the token (WG; nchunks <= 2048, checked by la_qk_prep). The launch and the LDS of the column sums read it here.
struct TokenShape { int nch; bool wg; };
TokenShape token_shape(int nchunks) {
    const int need = (nchunks + 63) / 64;                          // chunks per lane with one wave per token
    for (const int nch : {1, 2, 4, 8, 10})
        if (need <= nch) return {nch, false};
    return {nchunks <= 4 * 256 ? 4 : 8, true};
}
// ... and of the head kernel: a head's chunks sit on G = 1 << group_log2 lanes (head_dim <= 256: at most 5)
int head_group_log2(int head_dim) {
    int group_log2 = 0;
    while ((8 << group_log2) < head_dim) ++group_log2;
    return group_log2;
}

// Workgroups of a launch whose workgroup takes per_wg rows at a time (4: one per wave; 1: its waves share one). Mode 0: one per per_wg
// tokens; the e4m3 forms: one per round of per_wg tokens of ONE batch; the smooth forms: one per block of 4 parts of one batch.
dim3 grid_for(const QkPrepParams& p, int mode, int per_wg) {
    const int64_t blocks = mode == 0 ? (p.tokens + per_wg - 1) / per_wg
                                     : p.tokens / p.seqlen * (mode >= 3 ? p.part_blocks : (p.seqlen + per_wg - 1) / per_wg);
    return dim3(static_cast<unsigned>(blocks < kMaxGrid ? blocks : kMaxGrid));
}

// One launch. A smooth form that sums columns asks for their dynamic LDS first; hipErrorInvalidValue etc. of that call stay in
// hipGetLastError for the caller.
template <int MODE, class K, class... Extra>
void launch_kernel(K kfn, const QkPrepParams& p, int per_wg, hipStream_t stream, Extra... extra) {
    const size_t lds = MODE >= 3 && p.colsum_part ? static_cast<size_t>(qk_prep_sum_slots(p)) * 8 * 256 * sizeof(float) : 0;
    if (lds != 0 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)) != hipSuccess)
        return;
    hipLaunchKernelGGL(kfn, grid_for(p, MODE, per_wg), dim3(256), lds, stream, p, extra...);
}

template <int DT_IN, int DT_OUT, int MODE>
void launch_typed(const QkPrepParams& p, hipStream_t stream) {
    if (p.norm_mode == 1) {
        const TokenShape ts = token_shape(p.num_heads * p.head_dim / 8);
#define LA_QK_PREP_TOKEN(NCH, WG) \
        if (ts.nch == NCH && ts.wg == WG) launch_kernel<MODE>(la_qk_prep_token_kernel<DT_IN, DT_OUT, NCH, WG, MODE>, p, WG ? 1 : 4, stream)
        LA_QK_PREP_TOKEN(1, false);
        LA_QK_PREP_TOKEN(2, false);
        LA_QK_PREP_TOKEN(4, false);
        LA_QK_PREP_TOKEN(8, false);
        LA_QK_PREP_TOKEN(10, false);
        LA_QK_PREP_TOKEN(4, true);
        LA_QK_PREP_TOKEN(8, true);
#undef LA_QK_PREP_TOKEN
    } else {
        launch_kernel<MODE>(la_qk_prep_head_kernel<DT_IN, DT_OUT, MODE>, p, 4, stream, head_group_log2(p.head_dim));
    }
}

// The input-type ladder, once: f(DT) with the la_dtype of x as a compile-time constant.
template <class F>
void with_in_dtype(int in_dtype, F f) {
    if (in_dtype == 0) f(std::integral_constant<int, 0>());
    else if (in_dtype == 1) f(std::integral_constant<int, 1>());
    else f(std::integral_constant<int, 3>());
}

// mean[b][h][d] = (part[0][b][h][d] + part[1][b][h][d] + ...) / seqlen, added in index order: one thread per column
__global__ void __launch_bounds__(256) la_colsum_finish_kernel(const float* __restrict__ part, int n_parts, int64_t cols, int head_dim,
                                                                 int num_heads, float seqlen, float* __restrict__ mean, int64_t m_bs,
                                                                 int64_t m_hs) {
    const int64_t c = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (c >= cols) return;
    float acc = 0.f;
    for (int q = 0; q < n_parts; ++q) acc += part[q * cols + c];
    const int64_t bh = c / head_dim, b = bh / num_heads;
    mean[b * m_bs + (bh - b * num_heads) * m_hs + (c - bh * head_dim)] = acc / seqlen;
}

}  // namespace

// chunk slots of 8 columns per thread whose running sums live in LDS: the token kernel's NCH; the head kernel's passes of 64 / G heads,
// in whole batches of kHeadUnroll
int qk_prep_sum_slots(const QkPrepParams& p) {
    if (p.norm_mode == 1) return token_shape(p.num_heads * p.head_dim / 8).nch;
    const int per_batch = (64 >> head_group_log2(p.head_dim)) * kHeadUnroll;
    return (p.num_heads + per_batch - 1) / per_batch * kHeadUnroll;
}

// Templates are instantiated in the order they are named, and that is the order of the kernels in the code object: the cases below keep
// the order the kernels have had since each form was added, so that an assembly diff against an earlier build shows code changes only.
hipError_t launch_qk_prep(const QkPrepParams& p, int in_dtype, int out_dtype, int mode, hipStream_t stream) {
    (void)hipGetLastError();
    if (mode == 3) with_in_dtype(in_dtype, [&](auto dt) { launch_typed<decltype(dt)::value, 2, 3>(p, stream); });
    else if (mode == 4) with_in_dtype(in_dtype, [&](auto dt) { launch_typed<decltype(dt)::value, 2, 4>(p, stream); });
    else if (mode == 0)
        with_in_dtype(in_dtype, [&](auto dt) {
            if (out_dtype == 0) launch_typed<decltype(dt)::value, 0, 0>(p, stream);
            else launch_typed<decltype(dt)::value, 1, 0>(p, stream);
        });
    else
        with_in_dtype(in_dtype, [&](auto dt) {
            if (mode == 1) launch_typed<decltype(dt)::value, 2, 1>(p, stream);
            else launch_typed<decltype(dt)::value, 2, 2>(p, stream);
        });
    return hipGetLastError();
}

hipError_t launch_colsum_finish(const float* part, int n_parts, int batch, int num_heads, int head_dim, int seqlen, float* mean,
                                int64_t m_bs, int64_t m_hs, hipStream_t stream) {
    (void)hipGetLastError();
    const int64_t cols = static_cast<int64_t>(batch) * num_heads * head_dim;
    hipLaunchKernelGGL(la_colsum_finish_kernel, dim3(static_cast<unsigned>((cols + 255) / 256)), dim3(256), 0, stream, part, n_parts, cols,
                       head_dim, num_heads, static_cast<float>(seqlen), mean, m_bs, m_hs);
    return hipGetLastError();
}

}  // namespace la
