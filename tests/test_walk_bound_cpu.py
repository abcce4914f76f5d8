"""CPU: the longest dense key range ONE launch of the hand-scheduled kernels takes, per element type and head dim, pinned at its edge.

``la_fwd_workspace_bytes`` is pure arithmetic (no HIP call): up to the bound it answers the unsplit size, one key tile further the
size of a split into two runs (``dense_split`` of la_api.hip: n = 2, chunk_tiles = ceil(k_tiles / 2)). The bound is where the LDS a
launch needs (la_fwd_shell.h: rings, meta words, walk buffers, tile-address table, parameter block) passes 160 KiB, so this holds the
one layout function to the byte. ``tests/golden/walk_bounds.json`` was written by this file (``python tests/test_walk_bound_cpu.py
OUT.json``) on the commit BEFORE the two shells' size formulas were merged; the same fixture holds on both sides."""
import ctypes
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from liteattention_amd import _cabi  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "walk_bounds.json")
DTYPES = {"bf16": _cabi.LA_DTYPE_BF16, "e4m3": _cabi.LA_DTYPE_FP8_E4M3}
HEAD_DIMS = (64, 96, 128, 192, 256)
B, SQ, H, HK = 1, 64, 2, 1            # the sizes of the partial O / LSE of a split; they do not move the bound
SCHED = 1024                          # the ticket counters


def workspace_bytes(lib, dtype, head_dim, seqlen_k):
    a = _cabi.LaFwdArgs()
    a.struct_size = ctypes.sizeof(_cabi.LaFwdArgs)
    a.dtype = DTYPES[dtype]
    a.batch, a.seqlen_q, a.seqlen_k, a.num_heads, a.num_heads_k, a.head_dim, a.head_dim_v = B, SQ, seqlen_k, H, HK, head_dim, head_dim
    return lib.la_fwd_workspace_bytes(ctypes.byref(a))


def unsplit_bytes(dtype, head_dim, k_tiles):
    return SCHED + (B * HK * k_tiles * 64 * (128 if head_dim == 96 else head_dim) if dtype == "e4m3" else 0)      # e4m3: + the prepared V^T tiles


def split_bytes(dtype, head_dim, k_tiles, n):
    chunk_tiles = -(-k_tiles // n)
    partials = n * (((B * SQ * H * head_dim * 2 + 15) & ~15) + B * H * SQ * 4)          # 16-bit partial O + fp32 LSE per run
    return unsplit_bytes(dtype, head_dim, chunk_tiles) + partials                     # e4m3: the V^T tiles of ONE run


def measure(lib):
    """{dtype: {head_dim: the largest seqlen_k that answers the unsplit size}} (the LDS bytes grow with k_tiles: bisection)."""
    out = {}
    for dtype in DTYPES:
        out[dtype] = {}
        for d in HEAD_DIMS:
            lo, hi = 1, 1 << 16
            while lo < hi:
                mid = (lo + hi + 1) // 2
                lo, hi = (mid, hi) if workspace_bytes(lib, dtype, d, 64 * mid) == unsplit_bytes(dtype, d, mid) else (lo, mid - 1)
            out[dtype][str(d)] = 64 * lo
    return out


@pytest.mark.parametrize("head_dim", HEAD_DIMS)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_the_last_unsplit_key_length_and_the_first_split_one(dtype, head_dim):
    lib = _cabi.load()
    seqlen_k = json.load(open(FIXTURE))[dtype][str(head_dim)]
    assert seqlen_k % 64 == 0 and seqlen_k >= 64
    k_tiles = seqlen_k // 64
    for s in (seqlen_k - 63, seqlen_k):                                   # the whole last tile
        assert workspace_bytes(lib, dtype, head_dim, s) == unsplit_bytes(dtype, head_dim, k_tiles), s
    assert workspace_bytes(lib, dtype, head_dim, seqlen_k - 64) == unsplit_bytes(dtype, head_dim, k_tiles - 1)
    # one tile further: two runs of ceil((k_tiles + 1) / 2) tiles (e4m3 shows chunk_tiles in the bytes: the V^T tiles of one run)
    got = workspace_bytes(lib, dtype, head_dim, seqlen_k + 1)
    assert got == split_bytes(dtype, head_dim, k_tiles + 1, 2), (got, k_tiles)
    assert got != split_bytes(dtype, head_dim, k_tiles + 1, 3) and got != unsplit_bytes(dtype, head_dim, k_tiles + 1)
    # ... and a split stays the fewest equal runs that fit: 2 up to twice the bound, 3 behind it
    assert workspace_bytes(lib, dtype, head_dim, 2 * seqlen_k) == split_bytes(dtype, head_dim, 2 * k_tiles, 2)
    assert workspace_bytes(lib, dtype, head_dim, 2 * seqlen_k + 1) == split_bytes(dtype, head_dim, 2 * k_tiles + 1, 3)


if __name__ == "__main__":
    json.dump(measure(_cabi.load()), open(sys.argv[1], "w"), indent=1, sort_keys=True)
