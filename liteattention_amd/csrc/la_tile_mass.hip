// la_tile_mass.hip — the softmax mass of every walked key tile, in one pass over Q K^T (C-ABI: la_tile_mass).
//
// The share of a query row's softmax that key tile n carries is  mass_i[n] = sum over the tile's keys j of exp2(s_ij c - L2_i),  with
// c = softmax_scale * log2 e and L2_i = lse_i * log2 e of the launch whose probabilities are wanted. A row whose dropped tiles hold
// mass delta has |O' - O| <= 2 delta max|V|, so this number - not the margin - is what a skip costs. The kernel writes, per (q-tile,
// walked tile), the largest mass of a row (mass_max) and the mean over the q-tile's rows (mass_mean), and on request the margins of
// la_vote_margins from the same walk and the same scores: the calibrator wants both maps and the second Q K^T pass is what it saves.
//
// The skeleton is la_vote_margins.hip's: one workgroup of four waves per (batch, head, q-tile), a wave owns 32 * NQ query rows.
//   Q    B operands of v_mfma_f32_32x32x16, loaded once, in registers for the whole walk (4 NQ D / 16 registers).
//   K    tiles of 64 keys through two LDS stages at a pitch of 2 D + 16 bytes; the 16-byte global loads of tile t + 1 are carried in
//        registers across the MFMAs of tile t; one barrier per tile.
//   S^T  = K Q^T: a lane's 32 accumulators of the two 32x32 blocks are 32 keys of ONE query row, lanes l and l ^ 32 split the row's 64.
//   L2   one register per row (NQ per lane), loaded once. Rows at or past Sq and rows whose lse is not finite take +inf: every
//        probability of theirs is exp2(-inf) = 0, so they add exactly nothing to either output and the loop has no branch for them.
//   p    one FMA and one v_exp_f32 per score. A row's mass: the lane's 32 probabilities added in index order, key block 0 then 1,
//        then one half-wave exchange and add. Keys at or past Sk (tile Kt - 1 only) are -inf behind the product and add 0.
//   out  mass_max and the row sum of mass_mean are reduced over the wave's rows on the DPP datapath into lane 31, the four waves'
//        parts go through LDS (three outputs, double-buffered by tile parity: the ring's barrier orders them), thread 0 stores one
//        fp32 per output and tile. mass_mean divides by the rows the q-tile has, min(block_m, Sq - m_block block_m).
// Every element of every requested output is written once per launch: the tiles the walk does not visit are NaN in all of them (the
// walked-tile bitmap of la_vote_margins_common.h); the walk's FIRST tile has a mass and is NaN in the margins only. No atomics on
// global memory and a fixed order of every sum: two launches agree bit for bit. MARGINS false compiles the margins' arithmetic out.
// LDS: tile_mass_lds_bytes - la_vote_margins' plus 64 bytes; two workgroups per compute unit at every head dim.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "la_vote_margins_common.h"

namespace la {
namespace {

constexpr int kThreads = 256;
constexpr int kBN = 64;           // keys per tile (la_tiles.h: every 16-bit geometry)
constexpr float kLog2e = 1.4426950408889634f;

// The mass of one query row in this lane's 32 keys of the tile: probabilities in index order, key block 0 then 1. RAGGED: the tile
// holds keys at or past Sk (`valid` keys are real); their probability is 0 whatever the sign of c.
template <bool RAGGED>
__device__ __forceinline__ float row_mass(const f32x16 (&acc)[2], float c, float neg_l2, int valid, int lane) {
    float sum = 0.f;
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            float pr = fast_exp2(__builtin_fmaf(acc[g][e], c, neg_l2));
            if (RAGGED && 32 * g + 8 * (e >> 2) + (e & 3) + 4 * (lane >> 5) >= valid) pr = 0.f;
            sum += pr;
        }
    return sum;
}

template <bool F16, int D, int NQ, bool MARGINS>
__global__ __launch_bounds__(kThreads, 2) void la_tile_mass_kernel(const VoteMarginsParams p) {
    using E = Elem16<F16>;
    using X8 = typename E::x8;
    constexpr int KS = D / 16;                       // contraction steps
    constexpr int CPR = D / 8;                       // 16-byte chunks of a key row
    constexpr int PITCH = D * 2 + 16;                // bytes between two keys of a stage
    constexpr int STAGE = kBN * PITCH;
    constexpr int CH = kBN * CPR / kThreads;         // chunks of a tile a thread moves
    static_assert(kBN * CPR % kThreads == 0, "a tile is a whole number of chunks per thread");

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const ring = smem;
    const int k_tiles = p.k_tiles;
    const VoteWalk w = vote_walk_at<3>(smem + 2 * STAGE, k_tiles);            // parts of three outputs, tile count, walk, two bitmaps
    float* const part = w.part;                      // [margins, max, sum][parity][wave]
    int* const seq = w.seq;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int vid = xcd_work_id<64>();               // consecutive q-tiles of a head share an XCD's L2: they walk the same K
    const int m_block = vid % p.q_tiles, bh = vid / p.q_tiles, b = bh / p.num_heads, h = bh % p.num_heads;
    const uint16_t* const qb = static_cast<const uint16_t*>(p.q) + b * p.q_bs + h * p.q_hs;
    const uint16_t* const kb = static_cast<const uint16_t*>(p.k) + b * p.k_bs + (h / p.heads_per_k) * p.k_hs;
    const int64_t out_row = (static_cast<int64_t>(bh) * p.q_tiles + m_block) * k_tiles;
    float* const out_margin = MARGINS ? p.margins + out_row : nullptr;
    float* const out_max = p.mass_max != nullptr ? p.mass_max + out_row : nullptr;
    float* const out_mean = p.mass_mean != nullptr ? p.mass_mean + out_row : nullptr;
    const u32x4 zero = {0u, 0u, 0u, 0u};

    // ---- the walk: seq[0 .. n_tiles), and the bitmap of the walked tiles behind the first
    vote_walk_build<kThreads>(w, p.read_list, p.list_int16, static_cast<int64_t>(bh) * p.q_tiles + m_block, k_tiles, tid);

    // ---- Q and -L2: the wave's rows, once. Rows at or past Sq are zero rows (they vote, the forward's convention) without mass.
    X8 qf[NQ][KS];
    float neg_l2[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const int r = m_block * p.block_m + (wave * NQ + j) * 32 + (lane & 31);
        const uint16_t* const src = qb + static_cast<int64_t>(r) * p.q_rs + (lane >> 5) * 8;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const u32x4 v = r < p.seqlen_q ? *reinterpret_cast<const u32x4*>(src + s * 16) : zero;
            qf[j][s] = __builtin_bit_cast(X8, v);
        }
        const float lse = r < p.seqlen_q ? p.lse[static_cast<int64_t>(bh) * p.seqlen_q + r] : INFINITY;
        neg_l2[j] = __builtin_isfinite(lse) ? -(lse * kLog2e) : -INFINITY;
    }
    __syncthreads();
    const int n_tiles = vote_walk_mark<kThreads>(w, tid);
    if (MARGINS) vote_walk_fill_nan<kThreads>(w, out_margin, k_tiles, tid);
    if (out_max != nullptr) vote_walk_fill_nan<kThreads, true>(w, out_max, k_tiles, tid);
    if (out_mean != nullptr) vote_walk_fill_nan<kThreads, true>(w, out_mean, k_tiles, tid);
    const int rows = min(p.block_m, p.seqlen_q - m_block * p.block_m);

    // ---- K tiles: global -> registers -> LDS stage
    u32x4 kr[CH];
    auto fetch = [&](int n) {
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const int i = tid + kThreads * j, key = n * kBN + i / CPR;
            kr[j] = key < p.seqlen_k ? *reinterpret_cast<const u32x4*>(kb + static_cast<int64_t>(key) * p.k_rs + (i % CPR) * 8) : zero;
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const int i = tid + kThreads * j;
            *reinterpret_cast<u32x4*>(ring + buf * STAGE + (i / CPR) * PITCH + (i % CPR) * 16) = kr[j];
        }
    };
    fetch(seq[0]);
    stage(0);
    __syncthreads();

    const float c = p.scale_log2;
    float m_run[NQ];
    for (int t = 0; t < n_tiles; ++t) {
        const int n = seq[t];
        const bool more = t + 1 < n_tiles;
        if (more) fetch(seq[t + 1]);

        f32x16 acc[NQ][2];
#pragma unroll
        for (int j = 0; j < NQ; ++j)
#pragma unroll
            for (int g = 0; g < 2; ++g)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[j][g][e] = 0.f;
        const unsigned char* const kt = ring + (t & 1) * STAGE + (lane & 31) * PITCH + (lane >> 5) * 16;
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const X8 a = __builtin_bit_cast(X8, *reinterpret_cast<const u32x4*>(kt + g * 32 * PITCH + s * 32));
#pragma unroll
                for (int j = 0; j < NQ; ++j) acc[j][g] = E::mfma(a, qf[j][s], acc[j][g]);
            }
        // accumulator e of key block g: key 32 g + 8 (e / 4) + e % 4 + 4 (lane / 32) of the tile
        const int valid = p.seqlen_k - n * kBN;
        const bool ragged = valid < kBN;
        if (MARGINS && ragged) {
#pragma unroll
            for (int j = 0; j < NQ; ++j)
#pragma unroll
                for (int g = 0; g < 2; ++g)
#pragma unroll
                    for (int e = 0; e < 16; ++e)
                        if (32 * g + 8 * (e >> 2) + (e & 3) + 4 * (lane >> 5) >= valid) acc[j][g][e] = -INFINITY;
        }
        float d = -INFINITY, mx = 0.f, sm = 0.f;
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            if (MARGINS) {                           // la_vote_margins' arithmetic, operation for operation
                float m_loc = fmaxf(acc[j][0][0], acc[j][1][0]);
#pragma unroll
                for (int e = 1; e < 16; ++e) m_loc = fmaxf(m_loc, fmaxf(acc[j][0][e], acc[j][1][e]));
                m_loc = half_swap_max(m_loc);
                if (t > 0) {
                    d = fmaxf(d, (m_loc - m_run[j]) * c);
                    m_run[j] = fmaxf(m_run[j], m_loc);
                } else {
                    m_run[j] = m_loc;
                }
            }
            const float mass = half_swap_sum(ragged ? row_mass<true>(acc[j], c, neg_l2[j], valid, lane)
                                                    : row_mass<false>(acc[j], c, neg_l2[j], valid, lane));
            mx = fmaxf(mx, mass);
            sm += mass;
        }
        // lanes l and l ^ 32 hold the same rows: lanes 0 .. 31 are the wave's rows, each once
        if (MARGINS) d = max_into_lane31(d);
        mx = max_into_lane31(mx);
        sm = sum_into_lane31(sm);
        if (lane == 31) {
            if (MARGINS) part[(t & 1) * 4 + wave] = d;
            part[8 + (t & 1) * 4 + wave] = mx;
            part[16 + (t & 1) * 4 + wave] = sm;
        }
        if (more) stage((t + 1) & 1);
        __syncthreads();
        if (tid == 0) {
            const float* const pd = part + (t & 1) * 4;
            if (MARGINS && t > 0) out_margin[n] = fmaxf(fmaxf(pd[0], pd[1]), fmaxf(pd[2], pd[3]));
            if (out_max != nullptr) out_max[n] = fmaxf(fmaxf(pd[8], pd[9]), fmaxf(pd[10], pd[11]));
            if (out_mean != nullptr) out_mean[n] = ((pd[16] + pd[17]) + (pd[18] + pd[19])) / static_cast<float>(rows);
        }
    }
}

template <bool F16, int D, int NQ, bool MARGINS>
hipError_t launch_one(const VoteMarginsParams& p, hipStream_t stream) {
    auto* const kfn = la_tile_mass_kernel<F16, D, NQ, MARGINS>;
    const size_t lds = tile_mass_lds_bytes(D, p.k_tiles);
    const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(kfn, dim3(static_cast<unsigned>(p.batch * p.num_heads * p.q_tiles)), dim3(kThreads), lds, stream, p);
    return hipGetLastError();
}

// 256-row q-tiles exist up to head_dim 128 only (la_tiles.h)
template <bool F16, int D>
hipError_t launch_rows(const VoteMarginsParams& p, hipStream_t stream) {
    const bool margins = p.margins != nullptr;
    if constexpr (D <= 128) {
        if (p.block_m == 256) return margins ? launch_one<F16, D, 2, true>(p, stream) : launch_one<F16, D, 2, false>(p, stream);
    }
    return margins ? launch_one<F16, D, 1, true>(p, stream) : launch_one<F16, D, 1, false>(p, stream);
}

template <bool F16>
hipError_t launch_dim(const VoteMarginsParams& p, int head_dim, hipStream_t stream) {
    switch (head_dim) {
        case 64: return launch_rows<F16, 64>(p, stream);
        case 96: return launch_rows<F16, 96>(p, stream);
        case 128: return launch_rows<F16, 128>(p, stream);
        case 192: return launch_rows<F16, 192>(p, stream);
        case 256: return launch_rows<F16, 256>(p, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_tile_mass(const VoteMarginsParams& p, int dtype, int head_dim, hipStream_t stream) {
    if (p.lse == nullptr || (p.margins == nullptr && p.mass_max == nullptr && p.mass_mean == nullptr)) return hipErrorInvalidValue;
    (void)hipGetLastError();   // drop any stale sticky error of this thread: only OUR launch is reported
    return dtype == 1 ? launch_dim<true>(p, head_dim, stream) : launch_dim<false>(p, head_dim, stream);
}

}  // namespace la
