// la_vote_margins_fp8.hip — the skip vote's margin of every walked key tile for e4m3 operands (C-ABI: la_vote_margins_fp8).
//
// The e4m3 forward takes its vote on the fp32 accumulators of v_mfma_scale_f32_32x32x64_f8f6f4 with unit block scales and folds the
// descales into c = softmax_scale * log2 e * q_descale * k_descale (la_fwd_kernel_x64_fp8.hip). This kernel writes
// margin[n] = max over the q-tile's rows of (m_loc - m_prev) * c  from the same instruction on the same bytes: the map of
// la_vote_margins.hip at twice the matrix rate and half the K bytes, with no 16-bit copy of q or k.
//
// One workgroup of four waves per (batch, head, q-tile); a wave owns 32 * NQ query rows (NQ = 2: 256-row q-tiles at head dims 64 /
// 96 / 128; 1: 128-row ones at 192 / 256 - the e4m3 forward's geometry, la_tiles.h). The contraction runs in KS = ceil(D / 64) steps of
// 64 bytes; only head_dim 96 leaves its last step half empty (192 = 3 * 64).
//   Q    B operand, loaded once and resident: lane l holds row l % 32, bytes 64 s + 32 (l / 32) ... + 31 of step s - 8 registers per
//        (32-row block, step), 8 NQ KS in all (32 at D = 128 and at 256). The MFMA sums over (half-wave, byte) pairs of A and B alike,
//        so any assignment of head-dim bytes to them is a product as long as both operands use the same one; this one makes a lane's
//        operand 32 CONTIGUOUS bytes of a row, two 16-byte loads from global memory (Q) or LDS (K). Bytes at or past D are zeros and
//        are not read.
//   K    tiles of 64 keys x D bytes through a ring of two LDS stages, global -> registers -> LDS: every thread carries its 16-byte
//        chunks of tile t + 1 from before the MFMAs of tile t to behind them; one barrier per tile. A stage row is 64 KS + 16 bytes:
//        16 KS + 4 dwords, an odd multiple of 4 banks, so the 16-byte reads of 16 consecutive keys (lane l reads key l % 32) cover
//        all 64 banks once. Bytes D ... 64 KS - 1 of every row (head_dim 96) are zeroed ONCE, in both stages - no stage store touches
//        them - because an e4m3 byte 0x7f there would be a NaN and 0 * NaN poisons the row. Keys at or past Sk are staged as zeros
//        and, in tile Kt - 1, masked to -inf behind the product.
//   S^T  = K Q^T: the accumulator layout of every 32x32 MFMA - a lane's 16 accumulators are 16 keys of ONE query row (column l % 32),
//        lanes l and l ^ 32 hold the two halves of the row's 32 keys. Both scale operands are the E8M0 byte 127 (2^0) in every byte.
//   m, out: as in la_vote_margins.hip - one running maximum per row, DPP maximum into lane 31, four part maxima through LDS by tile
//        parity, one fp32 store per tile by thread 0; NaN for the first walked tile and the unwalked ones from the shared prologue.
// Every element of the output row is stored exactly once, nothing is atomic on global memory, the order is fixed by the shape.
// LDS: 2 * 64 * (64 KS + 16) bytes of ring (18 KiB at D = 128, 34 KiB at 256) + 64 + 4 bytes per key tile.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "la_vote_margins_common.h"

namespace la {
namespace {

constexpr int kThreads = 256;
constexpr int kBN = 64;           // keys per tile (la_tiles.h: every e4m3 geometry)
constexpr int kUnitScales = 0x7f7f7f7f;      // E8M0 127 = 2^0, whichever byte the instruction selects

typedef int i32x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ i32x8 pack8(u32x4 lo, u32x4 hi) {
    return i32x8{static_cast<int>(lo[0]), static_cast<int>(lo[1]), static_cast<int>(lo[2]), static_cast<int>(lo[3]),
                 static_cast<int>(hi[0]), static_cast<int>(hi[1]), static_cast<int>(hi[2]), static_cast<int>(hi[3])};
}

template <int D, int NQ>
__global__ __launch_bounds__(kThreads, 2) void la_vote_margins_fp8_kernel(const VoteMarginsFp8Params pf) {
    constexpr int KS = (D + 63) / 64;                // contraction steps of 64 bytes
    constexpr int DP = KS * 64;                      // a staged key row, zero behind D
    constexpr int CPR = D / 16;                      // 16-byte chunks of a key row in global memory
    constexpr int PADC = (DP - D) / 16;              // ... of zeros behind them in a stage
    constexpr int PITCH = DP + 16;                   // bytes between two keys of a stage
    constexpr int STAGE = kBN * PITCH;
    constexpr int CHUNKS = kBN * CPR;
    constexpr int CH = (CHUNKS + kThreads - 1) / kThreads;     // chunks of a tile a thread moves (the last one guarded at D = 96)
    constexpr bool RAGGED = CHUNKS % kThreads != 0;
    static_assert(D % 32 == 0, "a half-wave's 32 bytes of a step are all inside the row or all behind it");
    const VoteMarginsParams& p = pf.m;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const ring = smem;
    const int k_tiles = p.k_tiles;
    const VoteWalk w = vote_walk_at(smem + 2 * STAGE, k_tiles);
    float* const part = w.part;
    int* const seq = w.seq;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5;
    const int vid = xcd_work_id<64>();               // consecutive q-tiles of a head share an XCD's L2: they walk the same K
    const int m_block = vid % p.q_tiles, bh = vid / p.q_tiles, b = bh / p.num_heads, h = bh % p.num_heads, hk = h / p.heads_per_k;
    const unsigned char* const qb = static_cast<const unsigned char*>(p.q) + b * p.q_bs + h * p.q_hs;
    const unsigned char* const kb = static_cast<const unsigned char*>(p.k) + b * p.k_bs + hk * p.k_hs;
    float* const out = p.margins + (static_cast<int64_t>(bh) * p.q_tiles + m_block) * k_tiles;
    const u32x4 zero = {0u, 0u, 0u, 0u};

    vote_walk_build<kThreads>(w, p.read_list, p.list_int16, static_cast<int64_t>(bh) * p.q_tiles + m_block, k_tiles, tid);

    // ---- the zero tail of every staged row, once for both stages
    if constexpr (PADC > 0) {
        for (int i = tid; i < 2 * kBN * PADC; i += kThreads)
            *reinterpret_cast<u32x4*>(ring + (i / PADC) * PITCH + D + (i % PADC) * 16) = zero;       // STAGE = kBN * PITCH: rows of both stages
    }

    // ---- Q: the wave's rows, once. Rows at or past Sq are zero rows and vote (the forward's convention).
    i32x8 qf[NQ][KS];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const int r = m_block * p.block_m + (wave * NQ + j) * 32 + (lane & 31);
        const unsigned char* const src = qb + static_cast<int64_t>(r) * p.q_rs + half * 32;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const bool in = r < p.seqlen_q && s * 64 + half * 32 + 32 <= D;          // bytes 64 s + 32 half ... + 31 lie inside the row
            const u32x4 lo = in ? *reinterpret_cast<const u32x4*>(src + s * 64) : zero;
            const u32x4 hi = in ? *reinterpret_cast<const u32x4*>(src + s * 64 + 16) : zero;
            qf[j][s] = pack8(lo, hi);
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
            const bool in = key < p.seqlen_k && (!RAGGED || i < CHUNKS);
            kr[j] = in ? *reinterpret_cast<const u32x4*>(kb + static_cast<int64_t>(key) * p.k_rs + (i % CPR) * 16) : zero;
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const int i = tid + kThreads * j;
            if (!RAGGED || i < CHUNKS) *reinterpret_cast<u32x4*>(ring + buf * STAGE + (i / CPR) * PITCH + (i % CPR) * 16) = kr[j];
        }
    };
    fetch(seq[0]);
    stage(0);
    __syncthreads();

    // c as the e4m3 forward's shell computes it: fp32, left to right, descales per (batch, K/V head), NULL = 1
    const float qd = pf.q_descale ? pf.q_descale[b * pf.qd_bs + hk * pf.qd_hs] : 1.f;
    const float kd = pf.k_descale ? pf.k_descale[b * pf.kd_bs + hk * pf.kd_hs] : 1.f;
    const float c = p.scale_log2 * qd * kd;
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
        const unsigned char* const kt = ring + (t & 1) * STAGE + (lane & 31) * PITCH + half * 32;
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const unsigned char* const src = kt + g * 32 * PITCH + s * 64;
                const i32x8 a = pack8(*reinterpret_cast<const u32x4*>(src), *reinterpret_cast<const u32x4*>(src + 16));
#pragma unroll
                for (int j = 0; j < NQ; ++j)
                    acc[j][g] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, qf[j][s], acc[j][g], 0, 0, 0, kUnitScales, 0, kUnitScales);
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
                        if (32 * g + 8 * (e >> 2) + (e & 3) + 4 * half >= valid) acc[j][g][e] = -INFINITY;
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
            const float* const pm = part + (t & 1) * 4;
            out[n] = fmaxf(fmaxf(pm[0], pm[1]), fmaxf(pm[2], pm[3]));
        }
    }
}

template <int D, int NQ>
hipError_t launch_one(const VoteMarginsFp8Params& p, hipStream_t stream) {
    auto* const kfn = la_vote_margins_fp8_kernel<D, NQ>;
    const size_t lds = vote_margins_fp8_lds_bytes(D, p.m.k_tiles);
    const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(kfn, dim3(static_cast<unsigned>(p.m.batch * p.m.num_heads * p.m.q_tiles)), dim3(kThreads), lds, stream, p);
    return hipGetLastError();
}

}  // namespace

// the q-tile is tile_shape(head_dim, 1): 256 rows (two 32-row blocks per wave) up to head_dim 128, 128 rows above
hipError_t launch_vote_margins_fp8(const VoteMarginsFp8Params& p, int head_dim, hipStream_t stream) {
    (void)hipGetLastError();   // drop any stale sticky error of this thread: only OUR launch is reported
    switch (head_dim) {
        case 64: return launch_one<64, 2>(p, stream);
        case 96: return launch_one<96, 2>(p, stream);
        case 128: return launch_one<128, 2>(p, stream);
        case 192: return launch_one<192, 1>(p, stream);
        case 256: return launch_one<256, 1>(p, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace la
