// la_vote_margins_common.h — what the margin kernels of both operand widths and the tile mass kernel share (la_vote_margins.hip,
// la_vote_margins_fp8.hip, la_tile_mass.hip): the maximum and the sum over a wave's query rows on the DPP datapath, and the prologue that turns a read-list row into the walk, the bitmap of the
// walked tiles and the NaN entries of the output row.
#pragma once
#include "la_fwd_common.h"

namespace la {

// One step of a maximum over lanes on the DPP datapath: lanes without a source keep their own value.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_max(float v) {
    const int x = __float_as_int(v);
    return fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(x, x, CTRL, ROW_MASK, 0xf, false)));
}
// Maximum over lanes 0 .. 31, valid in lane 31 (four row_shr steps scan each row of 16, row_bcast:15 carries row 0 into row 1).
__device__ __forceinline__ float max_into_lane31(float v) {
    v = dpp_max<0x111, 0xf>(v);
    v = dpp_max<0x112, 0xf>(v);
    v = dpp_max<0x114, 0xf>(v);
    v = dpp_max<0x118, 0xf>(v);
    return dpp_max<0x142, 0xa>(v);
}

// ... and a sum over lanes 0 .. 31 into lane 31 by the same steps: a lane without a source adds `old` = 0, so the row_shr steps are an
// inclusive scan of each row of 16 and every lane's value is counted once. A fixed order: two launches agree bit for bit.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float sum_into_lane31(float v) {
    v = dpp_add<0x111, 0xf>(v);
    v = dpp_add<0x112, 0xf>(v);
    v = dpp_add<0x114, 0xf>(v);
    v = dpp_add<0x118, 0xf>(v);
    return dpp_add<0x142, 0xa>(v);
}

// The walk storage of a workgroup behind its K ring (vote_margins_lds_bytes / vote_margins_fp8_lds_bytes: 64 bytes, then 4 bytes per
// key tile and two bitmaps over the key tiles; tile_mass_lds_bytes: 128 bytes in front, for the parts of three outputs).
struct VoteWalk {
    float* part;                 // [outputs][2][4] parts of the four waves, by tile parity (one output: the margins)
    int* n_tiles_slot;
    int* seq;                    // the key tiles in walk order
    unsigned* endflags;          // range ends of the list expansion
    unsigned* walked;            // the tiles that get a margin (adjacent to endflags)
};
template <int OUTPUTS = 1>
__device__ __forceinline__ VoteWalk vote_walk_at(unsigned char* base, int k_tiles) {
    constexpr int kHead = (OUTPUTS * 8 * 4 + 4 + 63) & ~63;      // the parts and the tile count, in whole lines of 64 bytes
    VoteWalk w;
    w.part = reinterpret_cast<float*>(base);
    w.n_tiles_slot = reinterpret_cast<int*>(w.part + OUTPUTS * 8);
    w.seq = reinterpret_cast<int*>(base + kHead);
    w.endflags = reinterpret_cast<unsigned*>(w.seq + ((k_tiles + 3) & ~3));
    w.walked = w.endflags + ((k_tiles + 31) >> 5);
    return w;
}

// seq[0 .. n_tiles) of q-tile `row_index` (= (b H + h) q_tiles + m_block): the expanded list row, or k_tiles - 1 ... 0. The caller
// puts a barrier between this and vote_walk_finish (the Q loads go in between).
template <int THREADS>
__device__ __forceinline__ void vote_walk_build(const VoteWalk& w, const void* read_list, int list_int16, int64_t row_index, int k_tiles,
                                                int tid) {
    const int words = (k_tiles + 31) >> 5, lane = tid & 63;
    for (int i = tid; i < 2 * words; i += THREADS) w.endflags[i] = 0u;         // endflags and walked are adjacent
    __syncthreads();
    if (read_list == nullptr) {
        for (int i = tid; i < k_tiles; i += THREADS) w.seq[i] = k_tiles - 1 - i;
        if (tid == 0) *w.n_tiles_slot = k_tiles;
    } else if (tid < 64) {
        const int64_t row = row_index * (k_tiles + 1);
        int n = 0;
        LA_WITH_LIST_TYPE(list_int16, n = expand_read_list(static_cast<const ListT*>(read_list) + row, w.seq, w.endflags, k_tiles, lane));
        if (lane == 0) *w.n_tiles_slot = n;
    }
}

// The bitmap of the tiles that get a margin (all walked ones but the first). Returns the number of walked tiles.
template <int THREADS>
__device__ __forceinline__ int vote_walk_mark(const VoteWalk& w, int tid) {
    const int n_tiles = *w.n_tiles_slot;
    for (int i = 1 + tid; i < n_tiles; i += THREADS) atomicOr(&w.walked[w.seq[i] >> 5], 1u << (w.seq[i] & 31));
    __syncthreads();
    return n_tiles;
}
// NaN into every element of an output row whose tile is not in that bitmap - and, KEEP_FIRST, is not the walk's first tile either (an
// output that has a value for every walked tile) - by the thread that owns it.
template <int THREADS, bool KEEP_FIRST = false>
__device__ __forceinline__ void vote_walk_fill_nan(const VoteWalk& w, float* out, int k_tiles, int tid) {
    const int first = KEEP_FIRST ? w.seq[0] : -1;
    for (int n = tid; n < k_tiles; n += THREADS)
        if (!((w.walked[n >> 5] >> (n & 31)) & 1u) && n != first) out[n] = __builtin_nanf("");
}
// Both, for a kernel whose one output is the margins.
template <int THREADS>
__device__ __forceinline__ int vote_walk_finish(const VoteWalk& w, float* out, int k_tiles, int tid) {
    const int n_tiles = vote_walk_mark<THREADS>(w, tid);
    vote_walk_fill_nan<THREADS>(w, out, k_tiles, tid);
    return n_tiles;
}

}  // namespace la
