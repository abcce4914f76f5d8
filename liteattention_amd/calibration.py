"""Threshold calibration for QK-Skip. The reference exposes only ``set_threshold`` and mentions
"error calibration" (/root/reference/README.md:14); this helper finds the threshold that reaches a target skip
fraction on a given sequence of attention inputs (e.g. the denoising steps of one layer).

``calibrate_error_schedule`` is the other calibrator: a threshold PER STEP (``LiteAttention.set_threshold_schedule``) under an error
bound per step - the reference's "assign different error bounds to different timesteps, with stricter bounds for earlier timesteps" -
with the error measured on the device by ``output_error`` (C-ABI ``la_output_error``: one pass, fp64)."""
from __future__ import annotations

import ctypes
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _cabi
from .lite_attention import LiteAttention


def run_steps(thr: float, qkv_at: Callable[[int], Tuple[torch.Tensor, torch.Tensor, torch.Tensor]], n_steps: int,
              max_batch_size: int = 1) -> Tuple[List[float], LiteAttention]:
    """Run ``n_steps`` calls at threshold ``thr``; returns the skip fraction of the READ list of every step."""
    att = LiteAttention(threshold=-1.0, max_batch_size=max_batch_size)
    att.threshold = thr
    trace = []
    for t in range(n_steps):
        q, k, v = qkv_at(t)
        trace.append(att.get_skip_fraction(batch=q.shape[0]))
        att(q, k, v)
    trace.append(att.get_skip_fraction())
    return trace, att


def calibrate_threshold(qkv_at, n_steps: int, target_skip: float, lo: float = -20.0, hi: float = -1e-3,
                        iters: int = 10, tol: float = 0.01, max_batch_size: int = 1):
    """Bisection on thr in [lo, hi) (constant over steps) so that the skip fraction of the list the LAST step
    reads hits ``target_skip`` +- tol. Skip fraction is monotone non-decreasing in thr. Returns (thr, trace)."""
    best = None
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        trace, _ = run_steps(mid, qkv_at, n_steps, max_batch_size)
        got = trace[-2]
        if best is None or abs(got - target_skip) < abs(best[2] - target_skip):
            best = (mid, trace, got)
        if abs(got - target_skip) <= tol:
            break
        if got < target_skip:
            lo = mid
        else:
            hi = mid
    return best[0], best[1]


# ---- output error on the device --------------------------------------------------------------------------------------------------
_ERR_DTYPES = {torch.bfloat16: _cabi.LA_DTYPE_BF16, torch.float16: _cabi.LA_DTYPE_FP16, torch.float32: _cabi.LA_DTYPE_FP32}
DEFAULT_ROWS_PER_BIN = 256         # the q-tile of the head_dim-128 kernels; also keeps the launch at many workgroups per compute unit


class ErrorStats:
    """``stats``: fp64 ``(B, H, nbins, 6)`` as ``la_output_error`` wrote it (``_cabi.LA_STAT_*`` index the last dimension). The
    properties are per ``(B, H)``, reduced over the bins in fp64 on the device; nothing here synchronises. A head whose reference is
    all zeros has ``rel_l1`` / ``rel_l2`` = nan (0 / 0) or inf. Elements where either operand is not finite are counted in
    ``nonfinite`` and take no part in the other numbers."""

    def __init__(self, stats: torch.Tensor, rows_per_bin: int):
        self.stats, self.rows_per_bin = stats, rows_per_bin

    def _sum(self, i: int) -> torch.Tensor:
        return self.stats[..., i].sum(dim=-1)

    @property
    def rel_l1(self) -> torch.Tensor:
        return self._sum(_cabi.LA_STAT_ABS_DIFF) / self._sum(_cabi.LA_STAT_ABS_REF)

    @property
    def rel_l2(self) -> torch.Tensor:
        return (self._sum(_cabi.LA_STAT_SQ_DIFF) / self._sum(_cabi.LA_STAT_SQ_REF)).sqrt()

    @property
    def max_abs(self) -> torch.Tensor:
        return self.stats[..., _cabi.LA_STAT_MAX_ABS_DIFF].amax(dim=-1)

    @property
    def nonfinite(self) -> torch.Tensor:
        return self._sum(_cabi.LA_STAT_NONFINITE).to(torch.int64)

    def per_bin(self, metric: str = "rel_l1") -> torch.Tensor:
        """``(B, H, nbins)``: the metric of every bin of ``rows_per_bin`` rows (with ``rows_per_bin`` = the q-tile: where along the
        sequence the error sits, i.e. where a must-do range would help)."""
        st = self.stats
        if metric == "rel_l1":
            return st[..., _cabi.LA_STAT_ABS_DIFF] / st[..., _cabi.LA_STAT_ABS_REF]
        if metric == "rel_l2":
            return (st[..., _cabi.LA_STAT_SQ_DIFF] / st[..., _cabi.LA_STAT_SQ_REF]).sqrt()
        if metric == "max_abs":
            return st[..., _cabi.LA_STAT_MAX_ABS_DIFF]
        if metric == "nonfinite":
            return st[..., _cabi.LA_STAT_NONFINITE].to(torch.int64)
        raise ValueError("metric: rel_l1, rel_l2, max_abs or nonfinite")


def output_error(out: torch.Tensor, ref: torch.Tensor, rows_per_bin: Optional[int] = None) -> ErrorStats:
    """Error statistics of ``out`` against ``ref``, both ``(B, S, H, D)`` device tensors (bf16, fp16 or fp32, independently; any batch /
    row / head strides that keep rows 16-byte aligned; last dimension contiguous; D a multiple of 8), in ONE pass over each by the
    ``la_output_error`` kernel: no temporaries, fp64 arithmetic, bit-reproducible. ``rows_per_bin``: rows per bin of the returned
    ``stats`` (default: 256, or S when shorter). Asynchronous on the current stream."""
    if out.dim() != 4 or out.shape != ref.shape:
        raise ValueError(f"out and ref must be (B, S, H, D) of one shape, got {tuple(out.shape)} and {tuple(ref.shape)}")
    if not (out.is_cuda and ref.is_cuda and out.device == ref.device):
        raise ValueError("out and ref must live on the same GPU (there is no CPU path)")
    if out.dtype not in _ERR_DTYPES or ref.dtype not in _ERR_DTYPES:
        raise TypeError(f"bf16, fp16 or fp32 operands, got {out.dtype} and {ref.dtype}")
    if out.stride(-1) != 1 or ref.stride(-1) != 1:
        raise ValueError("the last dimension must be contiguous")
    B, S, H, D = out.shape
    if D % 8 != 0:
        raise ValueError(f"the last dimension must be a multiple of 8 (16-byte loads), got {D}")
    rpb = min(S, DEFAULT_ROWS_PER_BIN) if rows_per_bin is None else int(rows_per_bin)
    if rpb <= 0:
        raise ValueError("rows_per_bin must be positive")
    stats = torch.empty(B, H, -(-S // rpb), _cabi.LA_STAT_COUNT, dtype=torch.float64, device=out.device)
    with torch.cuda.device(out.device):
        rc = _cabi.load().la_output_error(out.data_ptr(), _ERR_DTYPES[out.dtype], out.stride(0), out.stride(1), out.stride(2),
                                          ref.data_ptr(), _ERR_DTYPES[ref.dtype], ref.stride(0), ref.stride(1), ref.stride(2),
                                          B, S, H, D, rpb, stats.data_ptr(), torch.cuda.current_stream().cuda_stream)
    if rc != _cabi.LA_OK:
        raise RuntimeError(f"la_output_error: {_cabi.status_string(rc)}")
    return ErrorStats(stats, rpb)


# ---- error-bounded threshold schedules -------------------------------------------------------------------------------------------
class LiteAttentionBackend:
    """What ``calibrate_error_schedule`` drives: one ``LiteAttention`` on the inputs of ``qkv_at(t)``, errors from ``output_error``.
    A backend offers ``reset()``, ``snapshot()``, ``restore(snap)``, ``step(t, thr) -> out``, ``dense(t) -> out``,
    ``error(out, ref) -> float`` and ``skip_fraction()`` (of the list the next step reads); a CPU stand-in built on the oracle
    offers the same seven. ``calibrate_head_thresholds`` needs two more of its backend: ``step(t, thr)`` with an ``(H,)`` tensor of
    thresholds, one per head, and ``error_heads(out, ref) -> (H,)`` tensor (the worst batch entry of every head);
    ``skip_fraction_heads() -> (H,)`` is used for the trace when a backend has it."""

    def __init__(self, qkv_at: Callable[[int], Tuple[torch.Tensor, torch.Tensor, torch.Tensor]], metric: str = "rel_l1",
                 reduce: str = "max", max_batch_size: int = 1, list_dtype: Optional[torch.dtype] = None):
        if metric not in ("rel_l1", "rel_l2", "max_abs"):
            raise ValueError("metric: rel_l1, rel_l2 or max_abs")
        if reduce not in ("max", "mean"):
            raise ValueError("reduce: max or mean")
        self.qkv_at, self.metric, self.reduce = qkv_at, metric, reduce
        self.att = LiteAttention(threshold=-1.0, max_batch_size=max_batch_size, list_dtype=list_dtype)

    def reset(self):
        self.att.reset_skip_state()

    def snapshot(self):
        return self.att.snapshot()

    def restore(self, snap):
        self.att.restore(snap)

    def step(self, t: int, thr) -> torch.Tensor:
        if isinstance(thr, torch.Tensor):          # (H,): one threshold per head (a device tensor is taken as it is: no sync)
            self.att.set_head_thresholds(thr)
        else:
            self.att.set_threshold(thr)
        return self.att(*self.qkv_at(t))

    def dense(self, t: int) -> torch.Tensor:
        from .flash_attn_interface import flash_attn_func
        return flash_attn_func(*self.qkv_at(t))

    def error(self, out: torch.Tensor, ref: torch.Tensor) -> float:
        per_head = getattr(output_error(out, ref), self.metric)
        return float(per_head.max() if self.reduce == "max" else per_head.mean())

    def error_heads(self, out: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
        """``(H,)`` on the device: the metric per head, the worst entry of the batch. No synchronisation."""
        return getattr(output_error(out, ref), self.metric).amax(dim=0)

    def skip_fraction(self) -> float:
        return self.att.get_skip_fraction()

    def skip_fraction_heads(self) -> Optional[torch.Tensor]:
        """``(H,)`` on the device: the skipped fraction of the list the next step reads, per head over the batch. No synchronisation."""
        frac = self.att.get_skip_fraction_heads()
        return None if frac is None else frac.mean(dim=0)


def calibrate_error_schedule(qkv_at, n_steps: int, bounds: Sequence[float], metric: str = "rel_l1", reduce: str = "max",
                             lo: float = -20.0, hi: float = -1e-3, iters: int = 8, max_batch_size: int = 1,
                             backend=None) -> Tuple[List[float], List[dict]]:
    """A threshold per step such that the output of step t stays within ``bounds[t]`` of the DENSE output of the same step (``metric``
    per head: rel_l1, rel_l2 or max_abs; ``reduce``: the worst head or the mean). Greedy over the steps: the output of step t + 1
    depends on the thresholds only through the list step t wrote, so for t = 0 ... n - 2 the threshold of step t is bisected in
    [lo, hi) - every probe restores the snapshot taken before step t, runs step t at the probed value, runs step t + 1 and measures
    it against dense(t + 1), computed once - and step t is then committed at the HIGHEST PROBED value that met ``bounds[t + 1]`` (for
    a fixed read list a higher threshold keeps a subset of the tiles: the error is monotone up to rounding). If no probe did, ``lo``
    is probed; if that fails too the skips of earlier steps cannot be undone: ``lo`` is kept and ``trace[t + 1]["bound_met"]`` is
    False. The last entry repeats the one before it (its list is never read).

    Returns ``(thresholds, trace)``; ``trace[t]``: ``threshold``, ``error`` (of the committed run of step t against dense(t)),
    ``bound``, ``bound_met`` and ``skip_fraction`` (of the list step t read). ``LiteAttention.set_threshold_schedule(thresholds)``
    replays it. ``backend``: see ``LiteAttentionBackend`` (the default, built from ``qkv_at``)."""
    if n_steps < 2:
        raise ValueError("a schedule needs at least two steps (the threshold of a step shapes the list the NEXT one reads)")
    if len(bounds) != n_steps:
        raise ValueError(f"one bound per step: got {len(bounds)} for {n_steps} steps")
    if not lo < hi:
        raise ValueError("lo must be below hi")
    be = LiteAttentionBackend(qkv_at, metric, reduce, max_batch_size) if backend is None else backend
    be.reset()
    thresholds: List[float] = []
    trace: List[dict] = []
    dense_t = be.dense(0)
    for t in range(n_steps - 1):
        snap = be.snapshot()
        skip_t = be.skip_fraction()
        dense_next = be.dense(t + 1)
        bound = float(bounds[t + 1])

        def probe(thr: float) -> float:
            be.restore(snap)
            be.step(t, thr)
            return be.error(be.step(t + 1, thr), dense_next)      # the threshold of step t + 1 does not touch its own output

        a, b, best = lo, hi, None
        for _ in range(iters):
            mid = 0.5 * (a + b)
            if probe(mid) <= bound:
                best, a = mid, mid
            else:
                b = mid
        if best is None:
            best = lo                  # kept whether it meets the bound or not: the committed run of step t + 1 measures it
        be.restore(snap)
        out_t = be.step(t, best)
        err_t = be.error(out_t, dense_t)
        thresholds.append(best)
        trace.append(dict(threshold=best, error=err_t, bound=float(bounds[t]), bound_met=err_t <= float(bounds[t]), skip_fraction=skip_t))
        dense_t = dense_next
        del out_t
    t = n_steps - 1
    skip_t = be.skip_fraction()
    err_t = be.error(be.step(t, thresholds[-1]), dense_t)
    thresholds.append(thresholds[-1])
    trace.append(dict(threshold=thresholds[-1], error=err_t, bound=float(bounds[t]), bound_met=err_t <= float(bounds[t]), skip_fraction=skip_t))
    return thresholds, trace


def calibrate_head_thresholds(qkv_at, n_steps: int, bounds, metric: str = "rel_l1", lo: float = -20.0, hi: float = -1e-3,
                              iters: int = 8, max_batch_size: int = 1, backend=None) -> Tuple[torch.Tensor, List[dict]]:
    """``calibrate_error_schedule`` with one threshold per (step, head) instead of one per step: a table for
    ``LiteAttention.set_head_thresholds``. Heads are independent in attention - output, LSE and lists of head h depend on head h's
    threshold alone - so the greedy bisection of ``calibrate_error_schedule`` runs for all heads at once, at its launch count: for
    step t, ``a``, ``b`` and ``best`` are ``(H,)`` tensors on the device, a probe restores the snapshot taken before step t, runs step
    t with the vector of midpoints, runs step t + 1 and takes the error of every head against dense(t + 1) (``metric``: rel_l1, rel_l2
    or max_abs; the worst entry of the batch); the three tensors move by ``torch.where``, so nothing inside the loop synchronises
    with the host. Step t is committed, per head, at the HIGHEST PROBED value that met ``bounds[t + 1][h]`` - a point of the
    depth-``iters`` dyadic grid of [lo, hi), kept in fp64 and rounded to fp32 once - else at ``lo``. ``bounds``: one value per
    step, or ``(n_steps, H)``. The last row repeats the one before it (its list is never read).

    Returns ``(table, trace)``: ``table`` fp32 ``(n_steps, H)`` on the device; ``trace[t]``: ``(H,)`` device tensors ``threshold``,
    ``error`` (of the committed run of step t against dense(t)), ``bound``, ``bound_met`` (error <= bound) and ``skip_fraction`` (of
    the list step t read). ``backend``: see ``LiteAttentionBackend`` (the default, built from ``qkv_at``)."""
    if n_steps < 2:
        raise ValueError("a table needs at least two steps (the thresholds of a step shape the lists the NEXT one reads)")
    if not lo < hi:
        raise ValueError("lo must be below hi")
    be = LiteAttentionBackend(qkv_at, metric, "max", max_batch_size) if backend is None else backend
    be.reset()
    dense_t = be.dense(0)
    H, dev = dense_t.shape[2], dense_t.device
    bnd = torch.as_tensor(bounds, dtype=torch.float64, device=dev)
    if bnd.dim() == 1:
        bnd = bnd[:, None].expand(-1, H)
    if tuple(bnd.shape) != (n_steps, H):
        raise ValueError(f"bounds: one value per step or (n_steps, H) = ({n_steps}, {H}); got {tuple(bnd.shape)}")
    skip_heads = getattr(be, "skip_fraction_heads", None)

    def skipped():
        frac = None if skip_heads is None else skip_heads()
        return torch.zeros(H, dtype=torch.float32, device=dev) if frac is None else frac

    def entry(thr32, out, dense, t, skip):
        err = be.error_heads(out, dense).to(torch.float64)
        return dict(threshold=thr32, error=err, bound=bnd[t], bound_met=err <= bnd[t], skip_fraction=skip)

    rows: List[torch.Tensor] = []
    trace: List[dict] = []
    for t in range(n_steps - 1):
        snap = be.snapshot()
        skip_t = skipped()
        dense_next = be.dense(t + 1)
        a = torch.full((H,), float(lo), dtype=torch.float64, device=dev)
        b = torch.full((H,), float(hi), dtype=torch.float64, device=dev)
        best = a.clone()               # kept where no probe met the bound, whether lo meets it or not: the committed run measures it
        for _ in range(iters):
            mid = 0.5 * (a + b)
            mid32 = mid.to(torch.float32)
            be.restore(snap)
            be.step(t, mid32)
            ok = be.error_heads(be.step(t + 1, mid32), dense_next).to(torch.float64) <= bnd[t + 1]
            best = torch.where(ok, mid, best)
            a = torch.where(ok, mid, a)
            b = torch.where(ok, b, mid)
        row = best.to(torch.float32)
        be.restore(snap)
        out_t = be.step(t, row)
        rows.append(row)
        trace.append(entry(row, out_t, dense_t, t, skip_t))
        dense_t = dense_next
        del out_t
    t = n_steps - 1
    skip_t = skipped()
    rows.append(rows[-1])
    trace.append(entry(rows[-1], be.step(t, rows[-1]), dense_t, t, skip_t))
    return torch.stack(rows), trace


# ---- vote margins: the threshold of a target sparsity from one pass over Q K^T ----------------------------------------------------
_MARGIN_DTYPES = {torch.bfloat16: _cabi.LA_DTYPE_BF16, torch.float16: _cabi.LA_DTYPE_FP16}
MARGIN_HEAD_DIMS = (64, 96, 128, 192, 256)
_LOG2E = 1.4426950408889634


def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


def _check_margin_list(read_list: torch.Tensor, q: torch.Tensor, qt: int, kt: int):
    B, H = q.shape[0], q.shape[2]
    if read_list.dtype not in (torch.int32, torch.int16) or read_list.dim() != 4 or not read_list.is_contiguous():
        raise ValueError("read_list must be a contiguous int32 or int16 tensor [batch, heads, q_tiles, k_tiles + 1]")
    if read_list.device != q.device:
        raise ValueError("read_list must be on the device of q")
    if read_list.shape[0] < B or tuple(read_list.shape[1:]) != (H, qt, kt + 1):
        raise ValueError(f"read_list must be [>= {B}, {H}, {qt}, {kt + 1}] for these operands and flags, got {tuple(read_list.shape)}")


def _descale_fields(name: str, d: Optional[torch.Tensor], q: torch.Tensor, Hk: int):
    """(pointer, batch stride, head stride) of an fp32 ``(B, Hk)`` descale on q's device, any strides; None reads as 1.0."""
    if d is None:
        return None, 0, 0
    if d.dtype != torch.float32 or tuple(d.shape) != (q.shape[0], Hk) or d.device != q.device:
        raise ValueError(f"{name} must be an fp32 ({q.shape[0]}, {Hk}) tensor on the device of q, got {d.dtype} {tuple(d.shape)}")
    return d.data_ptr(), d.stride(0), d.stride(1)


def vote_margins(q: torch.Tensor, k: torch.Tensor, softmax_scale: Optional[float] = None, read_list: Optional[torch.Tensor] = None,
                 flags: Optional[int] = None, out: Optional[torch.Tensor] = None, *, q_descale: Optional[torch.Tensor] = None,
                 k_descale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The margin of the skip vote for every key tile a walk visits: fp32 ``(B, H, Qt, Kt)`` from one launch of ``la_vote_margins``
    - of ``la_vote_margins_fp8`` for ``float8_e4m3fn`` operands, which are read as they are, with the fp32 ``(B, Hk)`` ``q_descale`` /
    ``k_descale`` of the e4m3 forward (any strides, None = 1.0; the q-tile is the e4m3 forward's, which no flag changes). The
    contracts are in include/lite_attention_amd.h. A forward call at threshold ``thr`` over the same walk keeps exactly the
    tiles with ``margin > thr`` and each row's first tile; entries are NaN for that first tile and for tiles the walk does not visit.
    ``q`` (B, Sq, H, D), ``k`` (B, Sk, Hk, D): bf16 or fp16 device tensors with a contiguous last dimension and 16-byte aligned rows,
    D one of 64 / 96 / 128 / 192 / 256. ``read_list``: int32 or int16 ``[>= B, H, Qt, Kt + 1]`` in the geometry of ``flags``; None walks
    every tile, Kt - 1 ... 0. ``flags``: the geometry flags (LA_FLAG_HALF_VOTE, LA_FLAG_KERNEL_128ROW) of the forward the margins are
    for; None takes the host defaults, as a forward call does. ``out``: a contiguous fp32 ``(B, H, Qt, Kt)`` tensor to write into (every
    element is written). Asynchronous on the current stream."""
    if q.dim() != 4 or k.dim() != 4 or q.shape[0] != k.shape[0] or q.shape[3] != k.shape[3]:
        raise ValueError(f"q (B, Sq, H, D) and k (B, Sk, Hk, D) of one batch and head dim, got {tuple(q.shape)} and {tuple(k.shape)}")
    if not (q.is_cuda and k.device == q.device):
        raise ValueError("q and k must live on the same GPU (there is no CPU path; vote_margins_reference is the plain form)")
    fp8 = q.dtype == torch.float8_e4m3fn
    if (q.dtype not in _MARGIN_DTYPES and not fp8) or k.dtype != q.dtype:
        raise TypeError(f"bf16, fp16 or float8_e4m3fn operands of one dtype, got {q.dtype} and {k.dtype}")
    if not fp8 and (q_descale is not None or k_descale is not None):
        raise ValueError("q_descale / k_descale belong to float8_e4m3fn operands")
    if q.stride(-1) != 1 or k.stride(-1) != 1:
        raise ValueError("the last dimension must be contiguous")
    B, Sq, H, D = q.shape
    Sk, Hk = k.shape[1], k.shape[2]
    if D not in MARGIN_HEAD_DIMS:
        raise ValueError(f"head_dim must be one of {MARGIN_HEAD_DIMS}, got {D}")
    if min(B, Sq, Sk, Hk) < 1 or H % Hk != 0:
        raise ValueError(f"sizes must be positive and the heads of k must divide those of q, got {tuple(q.shape)} and {tuple(k.shape)}")
    f = (_cabi.default_flags() if flags is None else int(flags)) & _cabi.GEOMETRY_FLAGS
    bm, bn = _cabi.get_tile_sizes(D, 1, f) if fp8 else _cabi.get_tile_sizes(D, 2, f)
    f = 0 if fp8 else f
    qt, kt = _cdiv(Sq, bm), _cdiv(Sk, bn)
    if read_list is not None:
        _check_margin_list(read_list, q, qt, kt)
        if read_list.dtype == torch.int16:
            f |= _cabi.LA_FLAG_LIST_INT16
    if out is None:
        out = torch.empty(B, H, qt, kt, dtype=torch.float32, device=q.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, H, qt, kt) or not out.is_contiguous() or out.device != q.device:
        raise ValueError(f"out must be a contiguous fp32 ({B}, {H}, {qt}, {kt}) tensor on the device of q")
    if fp8:
        a, entry = _cabi.LaVoteMarginsFp8Args(), "la_vote_margins_fp8"
        a.struct_size = ctypes.sizeof(_cabi.LaVoteMarginsFp8Args)
        a.q_descale, a.q_descale_batch_stride, a.q_descale_head_stride = _descale_fields("q_descale", q_descale, q, Hk)
        a.k_descale, a.k_descale_batch_stride, a.k_descale_head_stride = _descale_fields("k_descale", k_descale, q, Hk)
    else:
        a, entry = _cabi.LaVoteMarginsArgs(), "la_vote_margins"
        a.struct_size, a.dtype = ctypes.sizeof(_cabi.LaVoteMarginsArgs), _MARGIN_DTYPES[q.dtype]
    a.q, a.k = q.data_ptr(), k.data_ptr()
    a.q_batch_stride, a.q_row_stride, a.q_head_stride = q.stride(0), q.stride(1), q.stride(2)
    a.k_batch_stride, a.k_row_stride, a.k_head_stride = k.stride(0), k.stride(1), k.stride(2)
    a.batch, a.seqlen_q, a.seqlen_k, a.num_heads, a.num_heads_k, a.head_dim = B, Sq, Sk, H, Hk, D
    a.softmax_scale = D ** -0.5 if softmax_scale is None else float(softmax_scale)
    a.flags = f
    a.read_list = None if read_list is None else read_list.data_ptr()
    a.margins = out.data_ptr()
    with torch.cuda.device(q.device):
        rc = getattr(_cabi.load(), entry)(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != _cabi.LA_OK:
        raise RuntimeError(f"{entry}: {_cabi.status_string(rc)}")
    return out


def _walk_of_row(row: Sequence[int], kt: int) -> List[int]:
    """The key tiles one read-list row walks, in order, under the clamps of the kernels' list expansion."""
    n_ranges = min(max(row[0], 2) // 2, (kt + 1) // 2)
    walk: List[int] = []
    for r in range(n_ranges):
        in_row = 2 + 2 * r <= kt                 # a pair whose end lies behind the row reads as (0, 0); the first start is always in it
        start = min(max(row[1 + 2 * r], 0), kt - 1) if in_row or r == 0 else 0
        end = min(max(row[2 + 2 * r], 0), kt - 1) if in_row else 0
        tiles = list(range(start, end - 1, -1))
        if r == 0 and not tiles:
            tiles = [start]                      # the first tile of the first range is always walked
        walk += tiles
    return walk[:kt]


def vote_margins_reference(q: torch.Tensor, k: torch.Tensor, softmax_scale: Optional[float] = None,
                           read_list: Optional[torch.Tensor] = None, block_m: int = 256, block_n: int = 64, *,
                           q_descale: Optional[torch.Tensor] = None, k_descale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``vote_margins`` written plainly in fp64 torch, on any device: fp64 ``(B, H, Qt, Kt)``. Scores of all rows against all keys,
    the largest per (row, key tile), then per q-tile the walk of its list row with one running maximum per row. Rows at or past Sq
    are zero rows, keys at or past Sk are -inf; the first tile walked and the tiles not walked are NaN. ``q_descale`` / ``k_descale``
    (``(B, Hk)``, None = 1.0): the margins of (batch, head) are scaled by ``c = softmax_scale log2 e qd kd`` of its K/V head, in fp64."""
    B, Sq, H, D = q.shape
    Sk, Hk = k.shape[1], k.shape[2]
    qt, kt = _cdiv(Sq, block_m), _cdiv(Sk, block_n)
    c = torch.full((B, Hk), (D ** -0.5 if softmax_scale is None else float(softmax_scale)) * _LOG2E, dtype=torch.float64)
    for d in (q_descale, k_descale):
        if d is not None:
            c = c * d.to(device="cpu", dtype=torch.float64)
    c = c.repeat_interleave(H // Hk, dim=1).tolist()
    q64 = torch.zeros(B, qt * block_m, H, D, dtype=torch.float64, device=q.device)
    q64[:, :Sq] = q.to(torch.float64)
    k64 = k.to(torch.float64).repeat_interleave(H // Hk, dim=2)
    s = torch.full((B, H, qt * block_m, kt * block_n), float("-inf"), dtype=torch.float64, device=q.device)
    s[..., :Sk] = torch.einsum("bqhd,bkhd->bhqk", q64, k64)
    m_loc = s.view(B, H, qt, block_m, kt, block_n).amax(dim=-1)             # (B, H, Qt, rows, Kt)
    out = torch.full((B, H, qt, kt), float("nan"), dtype=torch.float64, device=q.device)
    rows = None if read_list is None else read_list[:B].cpu().tolist()
    for b in range(B):
        for h in range(H):
            for m in range(qt):
                walk = list(range(kt - 1, -1, -1)) if rows is None else _walk_of_row(rows[b][h][m], kt)
                run = m_loc[b, h, m, :, walk[0]]
                for n in walk[1:]:
                    out[b, h, m, n] = (m_loc[b, h, m, :, n] - run).amax() * c[b][h]
                    run = torch.maximum(run, m_loc[b, h, m, :, n])
    return out


def _sorted_margins(margins: torch.Tensor, per_head: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(G, N)`` ascending with +inf behind the finite entries, and their number ``(G,)``; G = H groups of one head each, or 1."""
    if margins.dim() != 4:
        raise ValueError(f"margins must be (B, H, Qt, Kt), got {tuple(margins.shape)}")
    m = margins.permute(1, 0, 2, 3).reshape(margins.shape[1], -1) if per_head else margins.reshape(1, -1)
    finite = torch.isfinite(m)
    return torch.where(finite, m, torch.full_like(m, float("inf"))).sort(dim=-1).values, finite.sum(dim=-1)


def _threshold_at_count(srt: torch.Tensor, n: torch.Tensor, k: torch.Tensor) -> torch.Tensor:
    """fp32, of the shape of ``k`` - ``(G,)`` or ``(G, J)``: per group a value with exactly ``k`` of its ``n`` finite sorted margins at
    or below it - the midpoint of the k-th and the (k + 1)-th, one below the smallest for k = 0, one above the largest for k = n,
    -inf for a group without margins."""
    n2 = n.unsqueeze(-1)
    k2 = torch.minimum(k.reshape(k.shape[0], -1).clamp(min=0), n2)
    lo = srt.gather(-1, (k2 - 1).clamp(min=0))
    hi = srt.gather(-1, k2.clamp(max=srt.shape[-1] - 1))
    mid = (0.5 * (lo.double() + hi.double())).to(torch.float32)
    mid = torch.where(mid >= hi, lo, mid)              # neighbours one ulp apart: the midpoint rounds onto one of them
    thr = torch.where(k2 == 0, hi - 1.0, torch.where(k2 >= n2, lo + 1.0, mid))
    return torch.where(n2 == 0, torch.full_like(thr, float("-inf")), thr).to(torch.float32).reshape(k.shape)


def _descents(margins: torch.Tensor, read_list: Optional[torch.Tensor], per_head: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """The list writer names one tile more than the vote keeps wherever, inside one range of the walk, a kept tile is followed by a
    dropped one: the dropped tile closes the range it writes (INCLUSIVE end). Tile n follows tile n + 1 when both are walked and n + 1
    does not end a range of the read list; such a pair adds a tile at every thr with margin[n] <= thr < margin[n + 1] (+inf for a
    row's first tile, which is always kept). Returns the two ends of these pairs, ``(G, N)`` each, sorted, +inf where there is none."""
    B, H, Qt, Kt = margins.shape
    fin = torch.isfinite(margins)
    first, ends = torch.zeros_like(fin), torch.zeros_like(fin)
    if read_list is None:
        first[..., Kt - 1] = True
    else:
        rl = read_list[:B].long()
        first.scatter_(-1, rl[..., 1:2].clamp(0, Kt - 1), True)
        at = rl[..., 2::2]
        used = torch.arange(at.shape[-1], device=rl.device) < rl[..., :1].clamp(min=2) // 2
        ends = torch.zeros(B, H, Qt, Kt, dtype=torch.int32, device=rl.device).scatter_add_(-1, at.clamp(0, Kt - 1), used.int()) > 0
    inf = torch.full_like(margins[..., 1:], float("inf"))
    before = torch.where(fin[..., 1:], margins[..., 1:], inf)
    pair = fin[..., :-1] & (fin | first)[..., 1:] & ~ends[..., 1:] & (before > margins[..., :-1])
    out = []
    for x in (torch.where(pair, margins[..., :-1], inf), torch.where(pair, before, inf)):
        out.append((x.permute(1, 0, 2, 3).reshape(H, -1) if per_head else x.reshape(1, -1)).sort(dim=-1).values.contiguous())
    return out[0], out[1]


def _threshold_for_listed(margins: torch.Tensor, read_list: Optional[torch.Tensor], keep: float, per_head: bool):
    """``(thr, listed, walked)``, ``(G,)`` each: the threshold - a midpoint between neighbouring margins - at which the list written
    over this walk names the number of tiles nearest to ``keep * walked``, that number, and the tiles walked. Every candidate is
    priced exactly, listed(thr) = rows + #{margin > thr} + #{descents that straddle thr}, by two sorts and two searches: no host
    synchronisation, no forward call."""
    srt, n = _sorted_margins(margins, per_head)
    G, N = srt.shape
    rows = margins[..., 0].numel() // G                                  # every row has one first tile, always kept
    j = torch.arange(N + 1, device=srt.device).expand(G, -1)
    cand = _threshold_at_count(srt, n, j).contiguous()
    lows, highs = _descents(margins, read_list, per_head)
    listed = rows + (n.unsqueeze(-1) - j) + torch.searchsorted(lows, cand, right=True) - torch.searchsorted(highs, cand, right=True)
    walked = n + rows
    cost = (listed.double() - keep * walked.double().unsqueeze(-1)).abs()
    best = torch.where(j > n.unsqueeze(-1), torch.full_like(cost, float("inf")), cost).argmin(dim=-1, keepdim=True)
    return cand.gather(-1, best).squeeze(-1), listed.gather(-1, best).squeeze(-1), walked


def threshold_for_skip(margins: torch.Tensor, target_skip: float, per_head: bool = False):
    """The threshold at which ``target_skip`` of the walked non-first tiles - the finite entries of ``margins`` - have ``margin <=
    thr`` and are dropped from the list a forward call over the same walk writes: a quantile on the device, ``round(target_skip *
    n)`` of the n finite entries. The value returned is the MIDPOINT between the two neighbouring margins, so that the fp32 rounding
    of the forward's own vote cannot move a tile across it. ``per_head``: an fp32 ``(H,)`` device tensor, one quantile per head over
    the batch (for ``LiteAttention.set_head_thresholds``), computed without synchronising; else one float over everything."""
    if not 0.0 <= target_skip <= 1.0:
        raise ValueError("target_skip must lie in [0, 1]")
    srt, n = _sorted_margins(margins, per_head)
    thr = _threshold_at_count(srt, n, torch.round(target_skip * n.double()).long())
    return thr if per_head else float(thr[0])


def calibrate_skip_schedule(qkv_at, n_steps: int, targets: Sequence[float], per_head: bool = False, hi: float = -1e-3,
                            max_batch_size: int = 1, list_dtype: Optional[torch.dtype] = None, descales_at=None):
    """A threshold per step - per (step, head) with ``per_head`` - such that the list step t WRITES keeps ``1 - targets[t]`` of the
    tiles step t walked, without bisection: per step one margin pass over the list the step reads (``LiteAttention.vote_margins``),
    the threshold from the margins on the device, one forward call at it. What a written list names is a pure function of the
    margins and the threshold - each row's first tile, the tiles with ``margin > thr``, and the dropped tile that closes a range
    (the writer's inclusive end) - so every midpoint between neighbouring margins is priced exactly and the nearest is taken. A
    ``descales_at``: for ``float8_e4m3fn`` operands, a callable ``t -> dict`` of ``q_descale`` / ``k_descale`` / ``v_descale``; what it
    returns is handed to both the margin pass (which reads q's and k's) and the forward call of step t. A
    threshold is capped at ``hi`` (``set_threshold`` takes negative values only: a tile with a positive margin raised a row's maximum
    and is never dropped); the trace shows what was reached.

    Returns ``(thresholds, trace)`` as ``calibrate_error_schedule`` does: a list of floats for ``set_threshold_schedule``, or an fp32
    ``(n_steps, H)`` device tensor for ``set_head_thresholds``. ``trace[t]``: ``threshold``, ``target``, ``skip_fraction`` (of the
    list step t read), ``walked`` and ``kept`` (tiles step t walked / its written list names: floats, or ``(H,)`` device tensors
    with ``per_head``, which never synchronises)."""
    from .flash_attn_interface import skip_list_stats_heads
    if len(targets) != n_steps:
        raise ValueError(f"one target per step: got {len(targets)} for {n_steps} steps")
    if hi >= 0:
        raise ValueError("hi must be negative")
    att = LiteAttention(threshold=-1.0, max_batch_size=max_batch_size, list_dtype=list_dtype)
    thresholds, trace = [], []
    for t in range(n_steps):
        q, k, v = qkv_at(t)
        skip_heads = att.get_skip_fraction_heads(q.shape[0])
        descales = {} if descales_at is None else dict(descales_at(t))
        margins = att.vote_margins(q, k, **{name: d for name, d in descales.items() if name != "v_descale"})
        thr, _, walked = _threshold_for_listed(margins, att.current_read_list(), 1.0 - float(targets[t]), per_head)
        thr = thr.clamp(max=hi)
        if per_head:
            att.set_head_thresholds(thr)
        else:
            thr = float(thr[0])
            att.set_threshold(thr)
        att(q, k, v, **descales)
        kept = skip_list_stats_heads(att.current_read_list(), q.shape[0]).sum(dim=0)
        if per_head:
            skip = torch.zeros_like(thr) if skip_heads is None else skip_heads.mean(dim=0)
        else:
            walked, kept, skip = float(walked[0]), float(kept.sum()), 0.0 if skip_heads is None else float(skip_heads.mean())
        thresholds.append(thr)
        trace.append(dict(threshold=thr, target=float(targets[t]), skip_fraction=skip, walked=walked, kept=kept))
    return (torch.stack(thresholds) if per_head else thresholds), trace


# ---- tile mass: the softmax mass of every walked key tile, and the threshold of a mass budget ----------------------------------
class TileMass(NamedTuple):
    """What ``tile_mass`` returns: fp32 ``(B, H, Qt, Kt)`` each (fp64 from ``tile_mass_reference``); ``margins`` is None unless asked."""
    mass_max: torch.Tensor
    mass_mean: torch.Tensor
    margins: Optional[torch.Tensor] = None


def _lse_bhs(lse: torch.Tensor, B: int, H: int, Sq: int) -> torch.Tensor:
    """``lse`` as ``(B, H, Sq)``: given so, or as the ``(B, Sq, H)`` view of it."""
    if tuple(lse.shape) == (B, H, Sq):
        return lse
    if tuple(lse.shape) == (B, Sq, H):
        return lse.transpose(1, 2)
    raise ValueError(f"lse must be ({B}, {H}, {Sq}) or its ({B}, {Sq}, {H}) view, got {tuple(lse.shape)}")


def tile_mass(q: torch.Tensor, k: torch.Tensor, lse: torch.Tensor, softmax_scale: Optional[float] = None,
              read_list: Optional[torch.Tensor] = None, flags: Optional[int] = None, *, margins: bool = False,
              out: Optional[TileMass] = None) -> TileMass:
    """The share of a query row's softmax that every key tile of a walk carries, reduced over the rows of a q-tile: ``mass_max``
    (the largest of a row) and ``mass_mean`` (the mean over the q-tile's rows), fp32 ``(B, H, Qt, Kt)`` each, from one launch of
    ``la_tile_mass`` (contract in include/lite_attention_amd.h). ``lse``: fp32 ``(B, H, Sq)``, or the ``(B, Sq, H)`` view of it, the
    natural-log LSE of the attention call whose probabilities are meant (``return_softmax_lse=True``); rows whose lse is not finite
    count as 0. ``margins=True``: the same launch also writes ``vote_margins`` of the same arguments, bit for bit. Every tile the walk
    does not visit is NaN in all outputs; the first walked tile has a mass and is NaN in the margins only. If the tiles dropped from
    a row hold mass delta, its output moves by at most ``2 delta max|V|``. ``q``, ``k``, ``softmax_scale``, ``read_list`` and ``flags``
    as ``vote_margins`` takes them; bf16 and fp16 only (e4m3 operands have ``vote_margins`` alone). ``out``: a ``TileMass`` of
    contiguous fp32 tensors to write into. Asynchronous on the current stream."""
    if q.dim() != 4 or k.dim() != 4 or q.shape[0] != k.shape[0] or q.shape[3] != k.shape[3]:
        raise ValueError(f"q (B, Sq, H, D) and k (B, Sk, Hk, D) of one batch and head dim, got {tuple(q.shape)} and {tuple(k.shape)}")
    if not (q.is_cuda and k.device == q.device and lse.device == q.device):
        raise ValueError("q, k and lse must live on the same GPU (there is no CPU path; tile_mass_reference is the plain form)")
    if q.dtype not in _MARGIN_DTYPES or k.dtype != q.dtype:
        raise TypeError(f"bf16 or fp16 operands of one dtype, got {q.dtype} and {k.dtype}")
    if q.stride(-1) != 1 or k.stride(-1) != 1:
        raise ValueError("the last dimension must be contiguous")
    B, Sq, H, D = q.shape
    Sk, Hk = k.shape[1], k.shape[2]
    if D not in MARGIN_HEAD_DIMS:
        raise ValueError(f"head_dim must be one of {MARGIN_HEAD_DIMS}, got {D}")
    if min(B, Sq, Sk, Hk) < 1 or H % Hk != 0:
        raise ValueError(f"sizes must be positive and the heads of k must divide those of q, got {tuple(q.shape)} and {tuple(k.shape)}")
    if lse.dtype != torch.float32:
        raise TypeError(f"lse must be fp32, got {lse.dtype}")
    lse = _lse_bhs(lse, B, H, Sq).contiguous()
    f = (_cabi.default_flags() if flags is None else int(flags)) & _cabi.GEOMETRY_FLAGS
    bm, bn = _cabi.get_tile_sizes(D, 2, f)
    qt, kt = _cdiv(Sq, bm), _cdiv(Sk, bn)
    if read_list is not None:
        _check_margin_list(read_list, q, qt, kt)
        if read_list.dtype == torch.int16:
            f |= _cabi.LA_FLAG_LIST_INT16
    if out is None:
        maps = [torch.empty(B, H, qt, kt, dtype=torch.float32, device=q.device) for _ in range(3 if margins else 2)]
        out = TileMass(*maps)
    for t in (out.mass_max, out.mass_mean) + ((out.margins,) if margins else ()):
        if t is None or t.dtype != torch.float32 or tuple(t.shape) != (B, H, qt, kt) or not t.is_contiguous() or t.device != q.device:
            raise ValueError(f"out must hold contiguous fp32 ({B}, {H}, {qt}, {kt}) tensors on the device of q")
    a = _cabi.LaVoteMarginsArgs()
    a.struct_size, a.dtype = ctypes.sizeof(_cabi.LaVoteMarginsArgs), _MARGIN_DTYPES[q.dtype]
    a.q, a.k = q.data_ptr(), k.data_ptr()
    a.q_batch_stride, a.q_row_stride, a.q_head_stride = q.stride(0), q.stride(1), q.stride(2)
    a.k_batch_stride, a.k_row_stride, a.k_head_stride = k.stride(0), k.stride(1), k.stride(2)
    a.batch, a.seqlen_q, a.seqlen_k, a.num_heads, a.num_heads_k, a.head_dim = B, Sq, Sk, H, Hk, D
    a.softmax_scale = D ** -0.5 if softmax_scale is None else float(softmax_scale)
    a.flags = f
    a.read_list = None if read_list is None else read_list.data_ptr()
    a.margins = out.margins.data_ptr() if margins else None
    with torch.cuda.device(q.device):
        rc = _cabi.load().la_tile_mass(ctypes.byref(a), lse.data_ptr(), out.mass_max.data_ptr(), out.mass_mean.data_ptr(),
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != _cabi.LA_OK:
        raise RuntimeError(f"la_tile_mass: {_cabi.status_string(rc)}")
    return out if margins else TileMass(out.mass_max, out.mass_mean, None)


def tile_mass_reference(q: torch.Tensor, k: torch.Tensor, lse: torch.Tensor, softmax_scale: Optional[float] = None,
                        read_list: Optional[torch.Tensor] = None, block_m: int = 256, block_n: int = 64, *,
                        margins: bool = False) -> TileMass:
    """``tile_mass`` written plainly in fp64 torch, on any device (``block_m`` / ``block_n`` in the place of ``flags``, as
    ``vote_margins_reference`` has them): ``p = exp(s softmax_scale - lse)`` for all rows against all keys, summed per (row, key
    tile), then the maximum and the mean over each q-tile's rows. Rows at or past Sq and rows whose lse is not finite count as 0 (the
    mean divides by the rows the q-tile has), keys at or past Sk are -inf; tiles the walk of the q-tile's list row does not visit are
    NaN."""
    B, Sq, H, D = q.shape
    Sk, Hk = k.shape[1], k.shape[2]
    qt, kt = _cdiv(Sq, block_m), _cdiv(Sk, block_n)
    scale = D ** -0.5 if softmax_scale is None else float(softmax_scale)
    k64 = k.to(torch.float64).repeat_interleave(H // Hk, dim=2)
    s = torch.full((B, H, qt * block_m, kt * block_n), float("-inf"), dtype=torch.float64, device=q.device)
    s[:, :, :Sq, :Sk] = torch.einsum("bqhd,bkhd->bhqk", q.to(torch.float64), k64) * scale
    l64 = torch.full((B, H, qt * block_m), float("inf"), dtype=torch.float64, device=q.device)
    given = _lse_bhs(lse, B, H, Sq).to(torch.float64)
    l64[:, :, :Sq] = torch.where(torch.isfinite(given), given, torch.full_like(given, float("inf")))
    mass = torch.exp(s - l64[..., None]).view(B, H, qt, block_m, kt, block_n).sum(dim=-1)          # (B, H, Qt, rows, Kt)
    rows = torch.tensor([min(block_m, Sq - m * block_m) for m in range(qt)], dtype=torch.float64, device=q.device)
    mass_max, mass_mean = mass.amax(dim=3), mass.sum(dim=3) / rows[:, None]
    walked = torch.ones(B, H, qt, kt, dtype=torch.bool)
    if read_list is not None:
        lists = read_list[:B].cpu().tolist()
        walked = torch.zeros(B, H, qt, kt, dtype=torch.bool)
        for b in range(B):
            for h in range(H):
                for m in range(qt):
                    walked[b, h, m, _walk_of_row(lists[b][h][m], kt)] = True
    nan = torch.full_like(mass_max, float("nan"))
    walked = walked.to(q.device)
    ref = vote_margins_reference(q, k, softmax_scale, read_list, block_m, block_n) if margins else None
    return TileMass(torch.where(walked, mass_max, nan), torch.where(walked, mass_mean, nan), ref)


def _group(x: torch.Tensor, per_head: bool) -> torch.Tensor:
    """``(B, H, ...)`` -> ``(G, N)``: one group per head over the batch, or one group of everything."""
    return x.transpose(0, 1).reshape(x.shape[1], -1) if per_head else x.reshape(1, -1)


def _dropped_mass(margins: torch.Tensor, mass: torch.Tensor, thr: torch.Tensor, reduce: str, per_head: bool) -> torch.Tensor:
    """``(G,)`` fp64: the mass of the dropped set {finite margin <= thr} as ``threshold_for_mass`` counts it - the worst q-tile's sum
    (``max``) or the mean over the q-tiles of their sums (``mean``)."""
    t = thr.reshape(1, -1, 1, 1) if per_head else thr.reshape(1, 1, 1, 1)
    per_tile = torch.where(torch.isfinite(margins) & (margins <= t), mass.double(), torch.zeros_like(mass, dtype=torch.float64)).sum(dim=-1)
    return _group(per_tile, per_head).amax(dim=-1) if reduce == "max" else _group(per_tile, per_head).mean(dim=-1)


def threshold_for_mass(margins: torch.Tensor, mass: torch.Tensor, budget: float, reduce: str = "max", per_head: bool = False,
                       hi: float = -1e-3):
    """The largest threshold whose dropped set - the tiles with a finite ``margin <= thr`` - stays inside a mass ``budget``, from
    the two maps of one ``tile_mass(..., margins=True)`` pass: no forward call, no bisection, no host synchronisation.
    ``reduce="max"`` with ``mass = mass_max``: for EVERY q-tile the ``mass_max`` of its dropped tiles sums to at most ``budget`` - a
    bound on the dropped mass of every row (a sum of maxima is at least the maximum of the sums), hence ``|O' - O| <= 2 budget
    max|V|`` for every row. ``reduce="mean"`` with ``mass = mass_mean``: the mean over the q-tiles of the summed ``mass_mean`` of
    their dropped tiles is at most ``budget``. The value is the MIDPOINT between the last margin dropped and the first one kept, as
    ``threshold_for_skip`` returns it, capped at ``hi``. ``per_head``: an fp32 ``(H,)`` device tensor, one threshold per head over
    the batch; else one float. The forward's list writer also KEEPS the dropped tile that closes a range (its inclusive end), so the
    forward drops a subset of the set priced here: the budget is conservative."""
    if reduce not in ("max", "mean"):
        raise ValueError("reduce: max or mean")
    if margins.dim() != 4 or mass.shape != margins.shape:
        raise ValueError(f"margins and mass must be (B, H, Qt, Kt) of one shape, got {tuple(margins.shape)} and {tuple(mass.shape)}")
    if budget < 0 or hi >= 0:
        raise ValueError("budget must not be negative and hi must be negative")
    fin = torch.isfinite(margins)
    m = torch.where(fin, margins, torch.full_like(margins, float("inf")))
    w = torch.where(fin, mass.double(), torch.zeros_like(mass, dtype=torch.float64))
    srt, n = _sorted_margins(margins, per_head)
    inf = torch.full((1,), float("inf"), dtype=srt.dtype, device=srt.device)
    if reduce == "max":
        row_m, order = m.sort(dim=-1)                                      # per q-tile: its tiles in the order a rising threshold drops them
        over = (w.gather(-1, order).cumsum(dim=-1) > budget) & torch.isfinite(row_m)
        limit = _group(torch.where(over, row_m, inf).amin(dim=-1), per_head).amin(dim=-1)          # the first margin that breaks a q-tile's budget
    else:
        grp_m, order = _group(m, per_head).sort(dim=-1)
        q_tiles = margins[..., 0].numel() // srt.shape[0]
        fits = (_group(w, per_head).gather(-1, order).cumsum(dim=-1) / q_tiles <= budget) & torch.isfinite(grp_m)
        k0 = fits.sum(dim=-1, keepdim=True)
        limit = torch.where(k0 < n.unsqueeze(-1), grp_m.gather(-1, k0.clamp(max=grp_m.shape[-1] - 1)), inf).squeeze(-1)
    k = torch.searchsorted(srt, limit.unsqueeze(-1).contiguous(), right=False).squeeze(-1)       # margins strictly below the limit: ties drop together
    thr = _threshold_at_count(srt, n, torch.minimum(k, n)).clamp(max=hi)
    return thr if per_head else float(thr[0])


def calibrate_mass_schedule(qkv_at, n_steps: int, budgets: Sequence[float], reduce: str = "max", per_head: bool = False,
                            hi: float = -1e-3, max_batch_size: int = 1, list_dtype: Optional[torch.dtype] = None):
    """A threshold per step - per (step, head) with ``per_head`` - under a MASS budget per step, without bisection. Step t: one
    forward call over the list the step reads, for its LSE (a threshold does not touch the output or the LSE of its own call, only
    the list it writes; that list is discarded by restoring the snapshot taken before); one ``tile_mass(..., margins=True)`` pass
    under the same list; ``threshold_for_mass`` of ``budgets[t]``; and the committed forward call at that threshold, which writes the
    list step t + 1 reads. Two forward calls and one map pass per step, against the 2 ``iters`` + 1 forward calls per step of
    ``calibrate_error_schedule``, and a bound instead of a probe: with ``reduce="max"`` every row of step t loses at most
    ``budgets[t]`` of the softmax mass step t computed, so its output moves by at most ``2 budgets[t] max|V|`` against that.
    ``budgets[t]`` is INCREMENTAL: relative to what step t computed over the list it read, not to the dense softmax; a cumulative
    audit against the dense result is not made here (``calibrate_error_schedule`` measures one).

    Returns ``(thresholds, trace)``: a list of floats for ``set_threshold_schedule``, or an fp32 ``(n_steps, H)`` device tensor for
    ``set_head_thresholds``. ``trace[t]``: ``threshold``, ``budget``, ``predicted_mass`` (the mass of the dropped set as
    ``threshold_for_mass`` counts it) and ``skip_fraction`` (of the list step t read); floats, or ``(H,)`` device tensors with
    ``per_head``, which never synchronises."""
    if len(budgets) != n_steps:
        raise ValueError(f"one budget per step: got {len(budgets)} for {n_steps} steps")
    att = LiteAttention(threshold=-1.0, max_batch_size=max_batch_size, list_dtype=list_dtype)
    thresholds, trace = [], []
    for t in range(n_steps):
        q, k, v = qkv_at(t)
        skip_heads = att.get_skip_fraction_heads(q.shape[0])
        snap = att.snapshot()
        _, lse = att(q, k, v, return_softmax_lse=True)
        att.restore(snap)
        maps = att.tile_mass(q, k, lse, margins=True)
        mass = maps.mass_max if reduce == "max" else maps.mass_mean
        thr = threshold_for_mass(maps.margins, mass, float(budgets[t]), reduce, per_head, hi)
        predicted = _dropped_mass(maps.margins, mass, torch.as_tensor(thr, dtype=torch.float32, device=q.device), reduce, per_head)
        if per_head:
            att.set_head_thresholds(thr)
            skip = torch.zeros_like(thr) if skip_heads is None else skip_heads.mean(dim=0)
        else:
            predicted = float(predicted)
            att.set_threshold(thr)
            skip = 0.0 if skip_heads is None else float(skip_heads.mean())
        att(q, k, v)
        thresholds.append(thr)
        trace.append(dict(threshold=thr, budget=float(budgets[t]), predicted_mass=predicted, skip_fraction=skip))
    return (torch.stack(thresholds) if per_head else thresholds), trace
