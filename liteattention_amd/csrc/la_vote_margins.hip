// la_vote_margins.hip — the skip vote's margin of every walked key tile, in one pass over Q K^T (C-ABI: la_vote_margins).
//
// The forward's vote keeps tile n of a q-tile when  margin[n] = max over the q-tile's rows of (m_loc - m_prev) * c  exceeds the
// threshold (m_loc: the row's largest score in the tile, m_prev: its running maximum over the tiles walked before, c = softmax_scale *
// log2 e). This kernel writes that number for every tile a walk visits and nothing else: half the matrix work of the forward, no
// exponential, no V. A threshold for a target sparsity is then a quantile of its output (liteattention_amd/calibration.py).
//
// One workgroup of four waves per (batch, head, q-tile); a wave owns 32 * NQ query rows (NQ = 2: 256-row q-tiles, 1: 128-row ones).
//   Q    the wave's rows as B operands of v_mfma_f32_32x32x16 (lane l: row l % 32, head-dim elements 16 s + 8 (l / 32) ... + 7 of
//        contraction step s), loaded once from global memory and kept in registers for the whole walk: 4 NQ D / 16 registers.
//   K    tiles of 64 keys through a ring of two LDS stages. Every thread carries D / 32 chunks of 16 bytes of tile t + 1 in registers
//        from before the MFMAs of tile t to behind them, so the loads fly under the matrix work; one barrier per tile. A row of a stage
//        is 2 D + 16 bytes: the 16-byte reads of consecutive keys (the A operand: lane l reads key l % 32, chunk 2 s + l / 32) fall into
//        different banks. Keys at or past Sk are stored as zeros and, in tile Kt - 1, masked to -inf behind the product.
//   S^T  = K Q^T: a lane's 16 accumulators of a 32x32 block are 16 keys of ONE query row (column l % 32), lanes l and l ^ 32 hold the
//        two halves of the row's 32 keys. The row maximum of a tile is a maximum over 32 registers and one half-wave exchange.
//   m    the running maximum is one register per row (NQ per lane).
//   out  the tile's margin: a DPP reduction over the wave's rows (lane 31 ends with it), four part maxima through LDS (double-buffered
//        by tile parity: the ring's barrier orders them), one fp32 store per tile by thread 0.
// The output row is written exactly once per element and launch: thread 0 stores the walked tiles in walk order, and the tiles the
// walk does not visit - and its first tile, which has no margin - are set to NaN by the thread that owns them in a bitmap of the
// walked tiles. No atomics on global memory, a fixed reduction order: two launches agree bit for bit.
// LDS: 2 * 64 * (2 D + 16) bytes of ring (34 KiB at D = 128, 66 KiB at 256) + 4 bytes per key tile: two workgroups per compute unit
// at every head dim up to ~3 000 key tiles (2 waves per SIMD, 256 registers each), so one's loads hide under the other's MFMAs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "la_vote_margins_common.h"

namespace la {
namespace {

constexpr int kThreads = 256;
constexpr int kBN = 64;           // keys per tile (la_tiles.h: every 16-bit geometry)

template <bool F16, int D, int NQ>
__global__ __launch_bounds__(kThreads, 2) void la_vote_margins_kernel(const VoteMarginsParams p) {
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
    const VoteWalk w = vote_walk_at(smem + 2 * STAGE, k_tiles);               // part maxima, tile count, walk, two bitmaps
    float* const part = w.part;
    int* const seq = w.seq;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int vid = xcd_work_id<64>();               // consecutive q-tiles of a head share an XCD's L2: they walk the same K
    const int m_block = vid % p.q_tiles, bh = vid / p.q_tiles, b = bh / p.num_heads, h = bh % p.num_heads;
    const uint16_t* const qb = static_cast<const uint16_t*>(p.q) + b * p.q_bs + h * p.q_hs;
    const uint16_t* const kb = static_cast<const uint16_t*>(p.k) + b * p.k_bs + (h / p.heads_per_k) * p.k_hs;
    float* const out = p.margins + (static_cast<int64_t>(bh) * p.q_tiles + m_block) * k_tiles;
    const u32x4 zero = {0u, 0u, 0u, 0u};

    // ---- the walk: seq[0 .. n_tiles), and the bitmap of the tiles that get a margin
    vote_walk_build<kThreads>(w, p.read_list, p.list_int16, static_cast<int64_t>(bh) * p.q_tiles + m_block, k_tiles, tid);

    // ---- Q: the wave's rows, once. Rows at or past Sq are zero rows and vote (the forward's convention).
    X8 qf[NQ][KS];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const int r = m_block * p.block_m + (wave * NQ + j) * 32 + (lane & 31);
        const uint16_t* const src = qb + static_cast<int64_t>(r) * p.q_rs + (lane >> 5) * 8;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const u32x4 v = r < p.seqlen_q ? *reinterpret_cast<const u32x4*>(src + s * 16) : zero;
            qf[j][s] = __builtin_bit_cast(X8, v);
        }
    }
    __syncthreads();
    const int n_tiles = vote_walk_finish<kThreads>(w, out, k_tiles, tid);

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
        if (valid < kBN) {
#pragma unroll
            for (int j = 0; j < NQ; ++j)
#pragma unroll
                for (int g = 0; g < 2; ++g)
#pragma unroll
                    for (int e = 0; e < 16; ++e)
                        if (32 * g + 8 * (e >> 2) + (e & 3) + 4 * (lane >> 5) >= valid) acc[j][g][e] = -INFINITY;
        }
        float d = -INFINITY;
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
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
        d = max_into_lane31(d);
        if (lane == 31) part[(t & 1) * 4 + wave] = d;
        if (more) stage((t + 1) & 1);
        __syncthreads();
        if (tid == 0 && t > 0) {
            const float* const w = part + (t & 1) * 4;
            out[n] = fmaxf(fmaxf(w[0], w[1]), fmaxf(w[2], w[3]));
        }
    }
}

template <bool F16, int D, int NQ>
hipError_t launch_one(const VoteMarginsParams& p, hipStream_t stream) {
    auto* const kfn = la_vote_margins_kernel<F16, D, NQ>;
    const size_t lds = vote_margins_lds_bytes(D, p.k_tiles);
    const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(kfn, dim3(static_cast<unsigned>(p.batch * p.num_heads * p.q_tiles)), dim3(kThreads), lds, stream, p);
    return hipGetLastError();
}

// 256-row q-tiles exist up to head_dim 128 only (la_tiles.h)
template <bool F16, int D>
hipError_t launch_rows(const VoteMarginsParams& p, hipStream_t stream) {
    if constexpr (D <= 128) {
        if (p.block_m == 256) return launch_one<F16, D, 2>(p, stream);
    }
    return launch_one<F16, D, 1>(p, stream);
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

hipError_t launch_vote_margins(const VoteMarginsParams& p, int dtype, int head_dim, hipStream_t stream) {
    if (p.lse != nullptr) return launch_tile_mass(p, dtype, head_dim, stream);      // la_tile_mass: the kernel of la_tile_mass.hip
    (void)hipGetLastError();   // drop any stale sticky error of this thread: only OUR launch is reported
    return dtype == 1 ? launch_dim<true>(p, head_dim, stream) : launch_dim<false>(p, head_dim, stream);
}

}  // namespace la
