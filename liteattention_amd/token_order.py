"""Token orders for the attention of a (frames, height, width) latent grid.

Non-causal attention is permutation-equivariant over tokens: run on q, k and v in ANY common order it returns the rows of O and of the
LSE in that order. What the order decides is which tokens share a tile of the skip lists, and so how many tiles a vote can drop. In
raster order a 256-row q-tile of a wide frame is a stripe a few rows high; ``brick_order`` makes it a compact 3-D brick.

    order = brick_order((frames, height, width), device=x.device)             # once per grid
    hidden = order.gather(hidden)                                              # once, at the model boundary ...
    q = qk_prep(q_proj, w_q, eps, tables, positions=order)                     # ... then every layer only names the positions
    ...
    hidden = order.restore(hidden)                                             # once, at the exit

or, where the hidden states cannot be permuted, per layer: ``qk_prep(q_proj, ..., rows=order)`` (the gather fused into the prologue),
``order.gather(v)``, ``order.restore(o)``.

Limits. ``PreparedV`` / ``v_prep_tiles`` and packed variable-length calls take no map: gather V first. Skip lists, ``must_do_list`` and
``must_skip_list`` speak of rows in the order of the CALL; changing the order of a layer needs ``reset_skip_state()``. With ``bt = 1``
in every brick level a frame's tokens stay one contiguous row range, so frame-range must-do lists carry over unchanged.
What a brick order gains on a real model has not been measured; ``tools/token_order_bench.py`` measures a synthetic field."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from .qk_prep import _check_x, qk_prep as _qk_prep      # (the package's `qk_prep` attribute is the function)

DEFAULT_BRICKS = ((1, 16, 16), (1, 8, 8))


class TokenOrder:
    """A token order: ``src_rows[s]`` is the raster token (the row of the unordered tensor, and its rope position) that row s of the
    ordered tensor holds, ``dst_rows`` its inverse (None when ``src_rows`` is no permutation: a pruned or repeated selection), both
    int32 ``[S]`` on one device. ``grid`` / ``bricks``: what ``brick_order`` was asked for (None for a caller's table). Pass the object
    as ``rows=`` or ``positions=`` of the prologue calls."""

    def __init__(self, src_rows: torch.Tensor, src_seqlen: int, dst_rows: Optional[torch.Tensor] = None, grid=None, bricks=None):
        self.src_rows, self.dst_rows, self.src_seqlen, self.grid, self.bricks = src_rows, dst_rows, int(src_seqlen), grid, bricks

    def __len__(self):
        return self.src_rows.shape[-1]

    def __repr__(self):
        return f"TokenOrder({len(self)} rows of {self.src_seqlen}, grid={self.grid}, bricks={self.bricks}, device={self.src_rows.device})"

    @classmethod
    def from_rows(cls, src_rows: torch.Tensor, src_seqlen: int) -> "TokenOrder":
        """A caller's table: int32 ``[S]`` on the device the calls will run on, entries in ``[0, src_seqlen)``. Checked HERE, once, on
        the host (one copy of the table) - never per call: the kernels clamp what they read and report nothing. ``ValueError`` for an
        entry out of range, ``TypeError`` for another dtype. ``dst_rows`` is built when the table is a permutation of all
        ``src_seqlen`` rows."""
        if not isinstance(src_rows, torch.Tensor) or src_rows.dtype != torch.int32:
            raise TypeError(f"src_rows: an int32 tensor, got {getattr(src_rows, 'dtype', type(src_rows).__name__)}")
        if src_rows.dim() != 1:
            raise ValueError(f"src_rows must be [S], got {tuple(src_rows.shape)}")
        src_seqlen = int(src_seqlen)
        if src_seqlen < 1:
            raise ValueError(f"src_seqlen must be positive, got {src_seqlen}")
        host = src_rows.cpu().long()
        if host.numel() and (int(host.min()) < 0 or int(host.max()) >= src_seqlen):
            bad = int(((host < 0) | (host >= src_seqlen)).nonzero()[0])
            raise ValueError(f"src_rows[{bad}] = {int(host[bad])} is outside [0, {src_seqlen})")
        dst = None
        if host.numel() == src_seqlen and torch.equal(host.sort().values, torch.arange(src_seqlen)):
            dst = torch.empty(src_seqlen, dtype=torch.int32)
            dst[host] = torch.arange(src_seqlen, dtype=torch.int32)
            dst = dst.to(src_rows.device)
        return cls(src_rows.contiguous(), src_seqlen, dst)

    def _move(self, x, table, rows_in, out, what):
        _check_x(x, "torch.index_select(x, 1, rows)")
        if table is None:
            raise ValueError(f"{what}: this order is no permutation (it has no dst_rows)")
        if x.shape[1] != rows_in:
            raise ValueError(f"{what}: x has {x.shape[1]} rows, this order reads {rows_in}")
        return _qk_prep(x, norm=None, out=out, rows=table)

    def gather(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``out[:, s] = x[:, src_rows[s]]`` for x (B, src_seqlen, H, D) bf16 / fp16 / fp32 on the GPU: V, hidden states viewed as
        heads, any per-token tensor. One read and one write (``la_qk_prep_rows``, no norm, no tables); a 16-bit x gives an exact copy in
        its dtype, fp32 rounds to bf16 (or to the dtype of ``out``). ``out`` must not be x."""
        return self._move(x, self.src_rows, self.src_seqlen, out, "gather")

    def restore(self, o: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The inverse of ``gather``: ``out[:, src_rows[s]] = o[:, s]``, as the gather by ``dst_rows``. For O and for hidden states."""
        return self._move(o, self.dst_rows, len(self), out, "restore")

    def restore_lse(self, lse: torch.Tensor) -> torch.Tensor:
        """``lse`` (..., S) of a call in this order -> raster order. A torch index on the last dimension: small, off the hot path."""
        if self.dst_rows is None:
            raise ValueError("restore_lse: this order is no permutation (it has no dst_rows)")
        if lse.shape[-1] != len(self):
            raise ValueError(f"restore_lse: lse has {lse.shape[-1]} rows, this order {len(self)}")
        return lse.index_select(-1, self.dst_rows.to(lse.device))


def _brick_keys(grid: Tuple[int, int, int], bricks) -> torch.Tensor:
    """(T*H*W, 3 * (levels + 1)) int64: per raster token the coordinates of its brick at every level, outermost first, then (t, y, x)."""
    T, H, W = grid
    t = torch.arange(T).view(T, 1, 1).expand(T, H, W).reshape(-1)
    y = torch.arange(H).view(1, H, 1).expand(T, H, W).reshape(-1)
    x = torch.arange(W).view(1, 1, W).expand(T, H, W).reshape(-1)
    keys = []
    for bt, bh, bw in bricks:
        keys += [t // bt, y // bh, x // bw]
    return torch.stack(keys + [t, y, x], dim=1)


def brick_order(grid: Sequence[int], bricks: Sequence[Sequence[int]] = DEFAULT_BRICKS, device=None) -> TokenOrder:
    """The permutation of the ``T*H*W`` raster tokens of ``grid`` = (T, H, W) sorted by the coordinates of their outer brick, then of
    their inner brick, ..., then by (t, y, x). ``bricks``: the (bt, bh, bw) of each nesting level, outermost first; an inner level
    should divide the outer one (then every outer brick is a contiguous run of whole inner bricks). Extents the bricks do not divide
    give partial bricks at the edges - still a permutation. With the default ((1, 16, 16), (1, 8, 8)) an aligned run of 64 rows is one
    8 x 8 patch and one of 256 rows one 16 x 16 patch of a frame (where the frame has them whole): the k-tile and the q-tile of the
    256-row kernels. Built on the host, once per grid."""
    grid = tuple(int(g) for g in grid)
    bricks = tuple(tuple(int(v) for v in b) for b in bricks)
    if len(grid) != 3 or any(g <= 0 for g in grid):
        raise ValueError(f"grid must be three positive extents, got {grid}")
    if not bricks or any(len(b) != 3 or any(v <= 0 for v in b) for b in bricks):
        raise ValueError(f"bricks must be one or more (bt, bh, bw) of positive extents, got {bricks}")
    n = grid[0] * grid[1] * grid[2]
    if n > 0x7fffffff:
        raise ValueError(f"{n} tokens do not fit the int32 tables")
    keys = _brick_keys(grid, bricks)
    src = torch.arange(n)
    for c in range(keys.shape[1] - 1, -1, -1):                   # a stable sort per key, least significant first
        src = src[torch.sort(keys[src, c], stable=True).indices]
    dst = torch.empty(n, dtype=torch.int64)
    dst[src] = torch.arange(n)
    device = torch.device("cpu" if device is None else device)
    return TokenOrder(src.to(torch.int32).to(device), n, dst.to(torch.int32).to(device), grid, bricks)
