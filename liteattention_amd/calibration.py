"""Threshold calibration for QK-Skip. The reference exposes only ``set_threshold`` and mentions
"error calibration" (/root/reference/README.md:14); this helper finds the threshold that reaches a target skip
fraction on a given sequence of attention inputs (e.g. the denoising steps of one layer).

``calibrate_error_schedule`` is the other calibrator: a threshold PER STEP (``LiteAttention.set_threshold_schedule``) under an error
bound per step - the reference's "assign different error bounds to different timesteps, with stricter bounds for earlier timesteps" -
with the error measured on the device by ``output_error`` (C-ABI ``la_output_error``: one pass, fp64)."""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple

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
