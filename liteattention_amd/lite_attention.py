"""LiteAttention for MI355X: the per-layer owner of the ping-pong skip lists.

API-compatible with /root/reference/hopper/lite_attention.py (class, method, argument and attribute
names; defaults; list layout ``_skip_list[2, maxB, H, Qt, Kt+1]``; ``_phase``; ``threshold``), so
``from lite_attention import LiteAttention`` code runs unchanged. The attention itself is
``flash_attn_func`` -> ``torch.ops.lite_attention.fwd`` -> C-ABI ``la_fwd`` -> the gfx950 HIP kernel;
list construction lives in ``skip_lists.py``.

Behavioural differences, all fixes of reference defects:
  B-1  ``enable_skipping=False`` runs the dense kernel (reference: AttributeError, lite_attention.py:262-266)
  B-2  K-tile count from ``key.shape[1]`` (reference: from the query length, :121-122)
  B-3  ``calc_percentage`` is the true listed fraction (reference returns about -1, :61-85)
  B-4  ``must_skip_list`` in README format, caller's list untouched, nothing printed (:126-145)
  B-6  must-do list handed to the kernel as one cached row (reference: 4-D repeat + H2D per call, :239-241)
"""
from __future__ import annotations

import os
from typing import Optional, Sequence, Tuple, Union

import torch

from . import _cabi
from . import skip_lists as _sl
from .flash_attn_interface import flash_attn_func, get_tile_sizes

Tensor = torch.Tensor


def _verbose() -> bool:
    return os.getenv("LITE_ATTENTION_VERBOSE", "FALSE") != "FALSE"


class LiteAttention:
    """QK-Skip attention with internally managed read/write skip lists.

    Args mirror the reference (lite_attention.py:36): ``enable_skipping=True``, ``threshold=-10.0``
    (log2 domain, must be negative unless env LITE_ATTENTION_DEBUG is set), ``max_batch_size=4`` (an upper bound: the lists are
    allocated for the batch actually seen and grow up to it, ``_skip_list[2, batch_seen, H, Qt, Kt+1]``).
    ``list_dtype`` (extension): element type of the lists, ``torch.int32`` or ``torch.int16`` - int16 halves the list state (the only
    state a layer keeps; INTEGRATION.md has the footprint table) and changes no result; default: LA_LIST_DTYPE in the environment, else int32.
    One instance per attention layer; not thread-safe (README.md:162-172)."""

    def __init__(self, enable_skipping: bool = True, threshold: float = -10.0, max_batch_size: int = 4,
                 list_dtype: Optional[torch.dtype] = None):
        self.list_dtype = _sl.check_list_dtype(_cabi.default_list_dtype() if list_dtype is None else list_dtype, 0)
        self._skip_list: Optional[Tensor] = None   # [2, max_batch, H, Qt, Kt+1] of list_dtype
        self._phase = 0                            # index of the buffer the NEXT call reads
        self._shape_key = None                     # what the lists were built for
        self._must_do_rows = {}                    # (tokens, block_n, row width, device) -> device row (LRU, _MUST_DO_ROWS_MAX)
        self._last_percentage = 0.0
        self._threshold_schedule: Optional[Tuple[float, ...]] = None   # per-step thresholds (set_threshold_schedule); None = the constant
        self._step = 0                             # calls that used the lists since they were last (re)initialised
        self._head_thresholds: Optional[Tensor] = None   # fp32 (H,) or (n_steps, H) (set_head_thresholds); None = the scalar threshold(s)
        self._head_thresholds_dev = {}             # device -> copy of a table that was given on the host (made at the first call there)
        self.enable_skipping = enable_skipping
        self.max_batch_size = max_batch_size
        self.set_threshold(threshold)

    # ---- reference-compatible static helpers -------------------------------------------------
    @staticmethod
    def ceil_div(x, y):
        return _sl.cdiv(x, y)

    @staticmethod
    def get_MN(head_dim, element_size, v_colmajor=False):
        """(kTileM, kTileN) of the kernel, from ``la_get_tile_sizes`` (one table shared with the HIP code;
        the reference hand-copies it, lite_attention.py:87-111 vs tile_size.h:10-62)."""
        # v_colmajor: accepted and ignored. In the reference it only switches the fp8 head_dim-128 tile (224 -> 192 keys,
        # tile_size.h:55) - and only on the Python side: its op passes v_colmajor = false to tile_size_fwd_sm90 and requires
        # v.stride(-1) == 1 (flash_api.cpp:413,728), so a column-major V never reaches its kernel. This build's tiles do not
        # depend on the layout of V.
        return get_tile_sizes(head_dim, element_size)

    @staticmethod
    def calc_percentage(read_list: Tensor) -> float:
        """Fraction of tiles that are listed, i.e. NOT skipped (what lite_attention.py:61-85 intended)."""
        return _sl.listed_fraction(read_list)

    @staticmethod
    def init_skip_list(batch, seq_len, heads, head_dim, v_colmajor, dtype, device, must_skip_list=None,
                       seq_len_k=None, list_dtype: torch.dtype = torch.int32) -> Tensor:
        """``[2, batch, heads, q_tiles, k_tiles+1]`` int32, rows ``[2, k_tiles-1, 0, ...]`` (:113-153).
        ``seq_len_k`` (extension) defaults to ``seq_len``; ``list_dtype`` (extension): ``torch.int16`` for lists of half the bytes."""
        _, bn, qt, kt = _sl.tile_geometry(seq_len, seq_len if seq_len_k is None else seq_len_k, head_dim,
                                          dtype.itemsize)
        row = None if must_skip_list is None else _sl.must_skip_row(must_skip_list, bn, kt)
        return _sl.new_skip_lists(batch, heads, qt, kt, device, row, list_dtype)

    @staticmethod
    def _expand_must_do_list(must_do_list, list_shape, query, value):
        """4-D ``[maxB, H, Qt, Kt+1]`` expansion kept for API parity (:214-242); ``__call__`` does not use it."""
        _, bn = get_tile_sizes(query.shape[-1], query.dtype.itemsize)
        row = _sl.must_do_row(must_do_list, bn, list_shape[3], query.device)
        return row.repeat(*list_shape[:3], 1).contiguous()

    # ---- list management ----------------------------------------------------------------------
    def _init_skip_list(self, query: Tensor, value: Tensor, must_skip_list: list = None, batch: Optional[int] = None) -> Tensor:
        """Both ping-pong buffers for ``batch`` sequences (default: the batch of ``query``). The reference always allocates
        ``max_batch_size`` (lite_attention.py:155-162, SURVEY Appendix B-7: 326 MB per layer at the Wan2.1 shape with the
        default 4, 13 GB over 40 layers); here the lists cover the batch actually seen and grow on demand up to
        ``max_batch_size`` (``_get_read_write_lists``), so a default-constructed object costs what ``max_batch_size=1`` would."""
        return self.init_skip_list(query.shape[0] if batch is None else batch, query.shape[1], query.shape[2], query.shape[3],
                                   False, query.dtype, query.device, must_skip_list, seq_len_k=value.shape[1],
                                   list_dtype=self.list_dtype)

    def _get_read_write_lists(self, query: Tensor, value: Tensor, must_skip_list: list = None
                              ) -> Tuple[Optional[Tensor], Optional[Tensor]]:
        """(read, write) views for this call; (re)builds the lists when any of seq lengths / heads /
        head_dim / dtype / device / list element type - or the tile geometry of the kernel that will run - changed (:179-200) and flips the
        ping-pong phase (:203-210). A batch larger than any seen so far (<= max_batch_size) grows the lists: the state of the
        sequences already tracked is kept, the new ones start from "all tiles listed"."""
        if not self.enable_skipping:
            return None, None
        # checked on EVERY call (the reference only checks at (re)init, :158, and would index past the lists)
        assert query.shape[0] <= self.max_batch_size, "batch size must be less than or equal to max_batch_size (modify max_batch_size in LiteAttention constructor)"
        # the tile sizes belong to the key: LA_FWD_KERNEL=v2 changes the q-tile of head_dim 128 from 256 to 128 rows, and lists
        # built for one geometry are mis-shaped for the other
        key = (query.shape[1], value.shape[1], query.shape[2], query.shape[3], query.dtype, query.device,
               get_tile_sizes(query.shape[3], query.dtype.itemsize), self.list_dtype)
        if self._skip_list is None or key != self._shape_key:
            self._skip_list = self._init_skip_list(query, value, must_skip_list)
            self._shape_key = key
            self._phase = 0
            self._step = 0
            if _verbose():
                print("[Warning]: reinitialized skip list during the forward pass")
        elif query.shape[0] > self._skip_list.shape[1]:
            # growth replaces the tensor: a HIP graph captured earlier keeps pointers into the OLD lists and would ping-pong on freed
            # memory. It cannot be allowed inside a capture, and graphs captured before it must be re-captured (or avoid it: preallocate()).
            if query.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the skip lists would have to grow (a larger batch than any seen so far) inside a HIP-graph capture: "
                                   "call preallocate(batch) before capturing")
            grown = self._init_skip_list(query, value, must_skip_list)
            grown[:, : self._skip_list.shape[1]] = self._skip_list
            self._skip_list = grown
        rd = self._phase
        self._phase = 1 - rd
        return self._skip_list[rd], self._skip_list[1 - rd]

    def _take_threshold(self, sparse: bool) -> float:
        """The threshold of the call whose lists were just handed out; a call that uses the lists advances the step counter (a dense
        call leaves it alone, as it leaves the lists alone). Without a schedule: ``self.threshold``, as ever."""
        thr = self.current_threshold() if sparse else self.threshold
        if sparse:
            self._step += 1
        return thr

    def _head_table_on(self, device) -> Tensor:
        """The table as the kernels read it: a device tensor is the caller's own (no copy, so an in-place rewrite is seen); a table
        given on the host is copied to ``device`` once and kept."""
        table = self._head_thresholds
        if table.device == device:
            return table
        if table.device.type != "cpu":
            raise ValueError(f"the head thresholds live on {table.device}, the call is on {device}")
        dev = self._head_thresholds_dev.get(device)
        if dev is None:
            dev = self._head_thresholds_dev[device] = table.to(device)
        return dev

    def _check_head_table(self, query: Tensor):
        """Before the lists of a call are handed out: a table for another number of heads is the caller's mistake, not a step."""
        table = self._head_thresholds
        if table is not None and table.shape[-1] != query.shape[2]:
            raise ValueError(f"the head thresholds are for {table.shape[-1]} heads, the query has {query.shape[2]}")
        if table is not None and table.device.type != "cpu" and table.device != query.device:
            raise ValueError(f"the head thresholds live on {table.device}, the call is on {query.device}")

    def _take_thresholds(self, query: Tensor, sparse: bool):
        """``(thr, _thr_head)`` of the call whose lists were just handed out: the scalar of ``_take_threshold`` and, with a table set
        and a call that uses the lists, the step's row of it on the query's device (``thr`` is then not read). One step is counted."""
        row = None
        if sparse and self._head_thresholds is not None:
            table = self._head_table_on(query.device)
            row = table if table.dim() == 1 else table[min(self._step, table.shape[0] - 1)]
        return self._take_threshold(sparse), row

    def preallocate(self, query: Tensor, value: Tensor, batch: Optional[int] = None, must_skip_list: list = None):
        """Size the lists for ``batch`` sequences (default ``max_batch_size``) of this shape NOW, so that no later call has to grow them:
        what a caller does before capturing calls into a HIP graph (a graph keeps the list pointers of its capture; growth replaces the
        tensor). The state of sequences already tracked is kept; (re)initialises like any shape change otherwise."""
        batch = self.max_batch_size if batch is None else batch
        assert batch <= self.max_batch_size, "batch size must be less than or equal to max_batch_size (modify max_batch_size in LiteAttention constructor)"
        key = (query.shape[1], value.shape[1], query.shape[2], query.shape[3], query.dtype, query.device,
               get_tile_sizes(query.shape[3], query.dtype.itemsize), self.list_dtype)
        if self._skip_list is None or key != self._shape_key:
            self._skip_list = self._init_skip_list(query, value, must_skip_list, batch=batch)
            self._shape_key, self._phase, self._step = key, 0, 0
        elif batch > self._skip_list.shape[1]:
            grown = self._init_skip_list(query, value, must_skip_list, batch=batch)
            grown[:, : self._skip_list.shape[1]] = self._skip_list
            self._skip_list = grown

    _MUST_DO_ROWS_MAX = 8          # distinct must_do_list values whose device rows are kept (least recently used go first)

    def _must_do_device_row(self, must_do_list, query: Tensor, width: int) -> Tensor:
        toks = (0, 0) if must_do_list is None else tuple(must_do_list)   # [0,0] = empty must-do (:267)
        _, bn = get_tile_sizes(query.shape[-1], query.dtype.itemsize)
        # the row depends on nothing but (tokens, tile size, row width, device): it survives list re-initialisation, reset and
        # load_state_dict, so a call captured in a HIP graph never needs the host-to-device copy that builds it
        key = (toks, bn, width, str(query.device))
        row = self._must_do_rows.pop(key, None)
        if row is None:
            row = _sl.must_do_row(toks, bn, width, query.device)
            while len(self._must_do_rows) >= self._MUST_DO_ROWS_MAX:
                self._must_do_rows.pop(next(iter(self._must_do_rows)))
        self._must_do_rows[key] = row                                    # (re)inserted last = most recently used
        return row

    # ---- the attention call -------------------------------------------------------------------
    def __call__(self, query: Tensor, key: Tensor, value: Tensor, scale: Optional[float] = None,
                 return_softmax_lse: bool = False, must_do_list: list = None, must_skip_list: list = None, *,
                 q_descale: Optional[Tensor] = None, k_descale: Optional[Tensor] = None,
                 v_descale: Optional[Tensor] = None, v_shift: Optional[Tensor] = None, lse_shift: Optional[Tensor] = None,
                 out_dtype: Optional[torch.dtype] = None, out_fp8=False) -> Union[Tensor, Tuple[Tensor, Tensor]]:
        """One attention call of a denoising step (:244-291).

        query (B, S, H, D) bf16; key/value (B, Sk, H, D). Returns out (B, S, H, D) — the reference
        docstring's (B, S, H*D) is wrong (Appendix B-5) — or ``(out, lse)`` with lse (B, H, S) fp32.
        ``must_do_list``: token ranges ``[start0, end0, ...]`` (descending) never dropped;
        ``must_skip_list``: token ranges dropped from the start, applied when the lists are (re)built.
        ``q/k/v_descale`` (keyword-only extension; the reference class cannot pass them): fp32
        ``(batch, nheads_k)`` dequantisation scales for e4m3 inputs, as ``flash_attn_func`` takes them.
        ``v_shift`` / ``lse_shift`` / ``out_dtype`` (keyword-only extension): the restoring pass of V and K smoothing
        (``attn_unshift``), applied to what the forward returns - behind its internal split-KV merge. ``v_shift`` fp32
        (batch, nheads_k, D): the vector subtracted from V (``SmoothedV``), added back to O; rows without keys stay 0.
        ``lse_shift`` fp32 (batch, nheads, S): ``q . c`` of ``SmoothedQK``, folded into the returned LSE. ``out_dtype``:
        bf16 / fp16 / fp32 of the returned O (fp32: what an output projection reads).
        ``out_fp8`` (keyword-only extension): True, or ``dict(heads_per_scale=..., descale=...)``: the restoring pass is
        ``attn_out_fp8`` and a ``v_prep.RowScaledE4m3`` (e4m3 data, its descale: the activation of an fp8 output projection) is
        returned in the place of O. Not together with ``out_dtype``.
        ``value`` may be a ``v_prep.PreparedV`` (``v_prep_tiles``, ``SmoothedV(tiles=True)``): e4m3 query / key, the launch runs on
        its workspace and a dense call is never split over the keys."""
        tiles = not isinstance(value, Tensor)
        if tiles:
            value.check_call(query, key)
        restore = v_shift is not None or lse_shift is not None or out_dtype is not None or out_fp8 is not False
        if restore:
            out_fp8 = self._check_restore(query, key, value, v_shift, lse_shift, out_dtype, out_fp8)
        self._check_head_table(query)
        read_list, write_list = self._get_read_write_lists(query, key, must_skip_list)
        must_do = None
        if read_list is not None:
            must_do = self._must_do_device_row(must_do_list, query, read_list.shape[3])
        extra = {}
        if q_descale is not None or k_descale is not None or v_descale is not None:      # only when given: the host-logic
            extra = dict(q_descale=q_descale, k_descale=k_descale, v_descale=v_descale)     # tests record the exact call
        if read_list is None and not tiles:
            # dense calls (enable_skip_optimization(False): the t2t / t2v / v2t calls of the text + video recipe, README.md:225-246) may be
            # split over the keys when they have fewer items than the device has workgroup slots: num_splits = -1 lets the op decide by
            # the reference's heuristic (flash_api.cpp:437, heuristics.h:25-58; the reference class passes nothing, i.e. 1: its default
            # build has no split kernel, hopper/setup.py:48)
            extra["num_splits"] = -1
        # the restoring pass reads the LSE for its empty-row rule: ask the forward for it whenever a shift is given
        want_lse = return_softmax_lse or v_shift is not None or lse_shift is not None
        if tiles:
            output = self._fwd_prepared_v(query, key, value, scale, read_list, write_list, must_do, want_lse, **extra)
        elif read_list is not None and self._head_thresholds is not None:
            # a table of thresholds per head: flash_attn_func keeps the reference's signature, which has no such argument, so the
            # call goes to mha_fwd directly - the call flash_attn_func makes for a 1-D must-do row, plus the step's row of the table
            from .flash_attn_interface import mha_fwd
            q, k, v = [x if x.stride(-1) == 1 else x.contiguous() for x in (query, key, value)]
            thr, thr_head = self._take_thresholds(query, True)
            out, lse, *_ = mha_fwd(q, k, v, softmax_scale=scale, attn_read_list=read_list, attn_must_do_list=must_do,
                                   attn_write_list=write_list, thr=thr, _must_do_is_1d=True, _thr_head=thr_head, **extra)
            output = (out, lse) if want_lse else out
        else:
            output = flash_attn_func(q=query, k=key, v=value, softmax_scale=scale, attn_read_list=read_list,
                                     attn_must_do_list=must_do, attn_write_list=write_list, thr=self._take_threshold(read_list is not None),
                                     return_softmax_lse=want_lse, **extra)
        if read_list is not None and _verbose():
            self._last_percentage = self.calc_percentage(read_list[: query.shape[0]])
            print(f"[Info]: Percentage of tiles skipped: {1.0 - self._last_percentage:.2%}")
        if restore:
            output = self._restore(output, want_lse, return_softmax_lse, scale, v_shift, lse_shift, out_dtype, out_fp8)
        return output

    def _fwd_prepared_v(self, query, key, value, scale, read_list, write_list, must_do, want_lse, q_windows=None, window_hook=None,
                        static_sched=False, **descales):
        """The forward for a ``PreparedV``: ``mha_fwd`` directly, as ``call_windowed`` reaches it, on the PreparedV's workspace."""
        from .flash_attn_interface import mha_fwd
        q, k = [x if x.stride(-1) == 1 else x.contiguous() for x in (query, key)]
        thr, thr_head = self._take_thresholds(query, read_list is not None)
        if thr_head is not None:                   # only when a table is set: the host-logic tests record the exact call
            descales = dict(descales, _thr_head=thr_head)
        out, lse, *_ = mha_fwd(q, k, value.as_v(), softmax_scale=scale, attn_read_list=read_list, attn_must_do_list=must_do,
                               attn_write_list=write_list, thr=thr, _must_do_is_1d=True,
                               _q_windows=q_windows, _window_hook=window_hook, _static_sched=static_sched, _v_prepared=value,
                               **descales)
        return (out, lse) if want_lse else out

    @staticmethod
    def _check_restore(query, key, value, v_shift, lse_shift, out_dtype, out_fp8=False):
        """The arguments of the restoring pass, before anything is launched. Returns ``out_fp8`` as None (off) or the keyword
        arguments of ``attn_out_fp8``."""
        B, S, H = query.shape[0], query.shape[1], query.shape[2]
        if out_fp8 is False or out_fp8 is None:
            out_fp8 = None
        else:
            if out_dtype is not None:
                raise ValueError(f"out_fp8 returns e4m3: out_dtype must be None, got {out_dtype}")
            out_fp8 = {} if out_fp8 is True else out_fp8
            if not isinstance(out_fp8, dict) or set(out_fp8) - {"heads_per_scale", "descale"}:
                raise ValueError(f"out_fp8: True, False or dict(heads_per_scale=..., descale=...), got {out_fp8!r}")
            from .v_prep import _check_out_fp8
            _check_out_fp8(torch.empty((B, S, H, value.shape[3]), device="meta"), out_fp8.get("heads_per_scale"), out_fp8.get("descale"),
                           None)
        if v_shift is not None and (v_shift.dtype != torch.float32 or tuple(v_shift.shape) != (B, key.shape[2], value.shape[3])):
            raise ValueError(f"v_shift must be fp32 (batch, nheads_k, D) = {(B, key.shape[2], value.shape[3])}, got {v_shift.dtype} "
                             f"{tuple(v_shift.shape)}")
        if lse_shift is not None and (lse_shift.dtype != torch.float32 or tuple(lse_shift.shape) != (B, H, S)):
            raise ValueError(f"lse_shift must be fp32 (batch, nheads, S) = {(B, H, S)}, got {lse_shift.dtype} {tuple(lse_shift.shape)}")
        if out_dtype not in (None, torch.bfloat16, torch.float16, torch.float32):
            raise ValueError(f"out_dtype: bf16, fp16 or fp32, got {out_dtype}")
        return out_fp8

    @staticmethod
    def _restore(output, have_lse, return_lse, scale, v_shift, lse_shift, out_dtype, out_fp8=None):
        from .v_prep import attn_out_fp8, attn_unshift
        o, lse = output if have_lse else (output, None)
        in_place = out_dtype is None or out_dtype == o.dtype
        fix_lse = lse_shift is not None and return_lse
        if out_fp8 is not None:
            res = attn_out_fp8(o, v_shift, lse=lse, lse_dot=lse_shift if fix_lse else None, softmax_scale=scale,
                               lse_out=lse if fix_lse else None, **out_fp8)
            out = res[0] if fix_lse else res
            return (out, lse) if return_lse else out
        if v_shift is None and in_place and not fix_lse:        # an LSE shift nobody asked the LSE of: nothing to do
            return (o, lse) if return_lse else o
        res = attn_unshift(o, v_shift, lse=lse, lse_dot=lse_shift if fix_lse else None, softmax_scale=scale, out=o if in_place else None,
                           out_dtype=out_dtype, lse_out=lse if fix_lse else None)
        out = res[0] if fix_lse else res
        return (out, lse) if return_lse else out

    def call_windowed(self, query: Tensor, key: Tensor, value: Tensor, q_windows, window_hook=None,
                      scale: Optional[float] = None, return_softmax_lse: bool = False, must_do_list: list = None,
                      must_skip_list: list = None, q_descale=None, k_descale=None, v_descale=None,
                      static_sched: bool = False) -> Union[Tensor, Tuple[Tensor, Tensor]]:
        """``__call__`` as several launches, one per q-tile window ``(first q-tile, count)`` (C-ABI ``q_tile_begin`` /
        ``q_tile_count``; tiles of ``get_MN``). Same lists, same ping-pong step, same results; rows of a window are
        final when its launch completes, and ``window_hook(i, out, row_begin, row_end)`` is called right after window i
        is enqueued — the head-sharded driver starts the xGMI all-gather of those rows there. The reference has one
        launch per call (flash_fwd_launch_template.h:359) and no such entry point."""
        from .flash_attn_interface import mha_fwd
        tiles = not isinstance(value, Tensor)
        if tiles:
            value.check_call(query, key)
        self._check_head_table(query)
        read_list, write_list = self._get_read_write_lists(query, key, must_skip_list)
        must_do = None
        if read_list is not None:
            must_do = self._must_do_device_row(must_do_list, query, read_list.shape[3])
        if tiles:
            return self._fwd_prepared_v(query, key, value, scale, read_list, write_list, must_do, return_softmax_lse, q_windows,
                                        window_hook, static_sched, q_descale=q_descale, k_descale=k_descale, v_descale=v_descale)
        q, k, v = [x if x.stride(-1) == 1 else x.contiguous() for x in (query, key, value)]
        thr, thr_head = self._take_thresholds(query, read_list is not None)
        extra = {} if thr_head is None else {"_thr_head": thr_head}      # only when a table is set
        out, lse, *_ = mha_fwd(q, k, v, q_descale=q_descale, k_descale=k_descale, v_descale=v_descale,
                               softmax_scale=scale, attn_read_list=read_list, attn_must_do_list=must_do,
                               attn_write_list=write_list, thr=thr, _must_do_is_1d=True,
                               _q_windows=q_windows, _window_hook=window_hook, _static_sched=static_sched, **extra)
        return (out, lse) if return_softmax_lse else out

    # ---- state control ------------------------------------------------------------------------
    def reset_skip_state(self):
        """Forget the lists; the next call starts from "all tiles listed" (:293-304)."""
        self._skip_list = None
        self._phase = 0
        self._shape_key = None
        self._last_percentage = 0.0
        self._step = 0

    def set_threshold(self, threshold: float):
        """Threshold must be negative unless env LITE_ATTENTION_DEBUG != "FALSE" (:306-313). Removes a threshold schedule: a constant
        is a constant."""
        if threshold >= 0 and os.getenv("LITE_ATTENTION_DEBUG", "FALSE") == "FALSE":
            raise ValueError("threshold must be negative when debug mode is not enabled")
        self.threshold = threshold
        self._threshold_schedule = None
        self._set_head_table(None)

    def _set_head_table(self, table: Optional[Tensor]):
        self._head_thresholds = table
        self._head_thresholds_dev = {}

    def set_head_thresholds(self, thresholds):
        """One vote threshold per QUERY head instead of one for all (extension: heads are independent in attention, so each can
        skip what it can afford; ``calibration.calibrate_head_thresholds`` finds such a table). ``None`` removes the table. Shape
        ``(H,)``: constant over the steps. Shape ``(n_steps, H)``: the i-th call that uses the skip lists takes row
        ``min(i, n_steps - 1)`` - the counting of ``set_threshold_schedule`` (dense calls do not count; ``reset_skip_state`` or a shape
        change restarts it). Values given on the HOST (a sequence, a CPU tensor) are checked like ``set_threshold``'s and copied to the
        device of the first call. A DEVICE tensor (float32) is taken as it is - no check, no copy, no synchronisation: the kernels
        read the caller's memory, which may be rewritten in place between calls or between replays of a captured graph. The last
        setter wins: ``set_threshold`` and ``set_threshold_schedule`` remove the table, this removes neither of theirs but is what
        a sparse call uses while it is set. A table whose H is not the query's is a ``ValueError`` at the call."""
        if thresholds is None:
            self._set_head_table(None)
            return
        on_device = isinstance(thresholds, Tensor) and thresholds.device.type != "cpu"
        table = thresholds if on_device else torch.as_tensor(thresholds, dtype=torch.float32)
        if table.dim() not in (1, 2) or table.numel() == 0:
            raise ValueError(f"head thresholds must have shape (H,) or (n_steps, H); got {tuple(table.shape)}")
        if on_device:
            if table.dtype != torch.float32:
                raise ValueError(f"a device table of head thresholds must be float32, got {table.dtype}")
        else:
            if bool((table >= 0).any()) and os.getenv("LITE_ATTENTION_DEBUG", "FALSE") == "FALSE":
                raise ValueError("threshold must be negative when debug mode is not enabled")
            if bool(torch.isnan(table).any()):
                raise ValueError("a head threshold is NaN")
            table = table.clone()
        self._set_head_table(table)

    def current_head_thresholds(self) -> Optional[Tensor]:
        """The ``(H,)`` row the next call that uses the skip lists will pass (a view of the table as it was set), or None."""
        table = self._head_thresholds
        if table is None or table.dim() == 1:
            return table
        return table[min(self._step, table.shape[0] - 1)]

    def set_threshold_schedule(self, thresholds: Optional[Sequence[float]]):
        """Per-step thresholds (extension; the reference's "error calibration" contribution, README.md:14, has no API there): the
        i-th call that uses the skip lists since the last ``reset_skip_state()`` - or since the lists were last re-initialised by a
        shape change - runs at ``thresholds[min(i, len - 1)]``. The threshold of call i shapes the list call i + 1 reads. Dense calls
        (``enable_skip_optimization(False)``) do not count. Every entry is checked like ``set_threshold``'s; ``None`` removes the
        schedule and the constant ``threshold`` applies again. ``calibration.calibrate_error_schedule`` finds such a schedule."""
        if thresholds is None:
            self._threshold_schedule = None
            self._set_head_table(None)
            return
        sched = tuple(float(t) for t in thresholds)
        if not sched:
            raise ValueError("an empty threshold schedule: pass None to remove the schedule")
        if any(t >= 0 for t in sched) and os.getenv("LITE_ATTENTION_DEBUG", "FALSE") == "FALSE":
            raise ValueError("threshold must be negative when debug mode is not enabled")
        self._threshold_schedule = sched
        self._set_head_table(None)                 # the last setter wins

    def current_threshold(self) -> float:
        """The threshold the next call that uses the skip lists will pass."""
        sched = self._threshold_schedule
        return self.threshold if sched is None else sched[min(self._step, len(sched) - 1)]

    def enable_skip_optimization(self, enable: bool = True):
        self.enable_skipping = enable

    # ---- additions: statistics and checkpoint/resume -------------------------
    def current_read_list(self) -> Optional[Tensor]:
        """The list the next call will read (= what the last call wrote)."""
        return None if self._skip_list is None else self._skip_list[self._phase]

    def get_skip_fraction(self, batch: Optional[int] = None) -> float:
        """Fraction of tiles the next call skips (device reduction; synchronises)."""
        rl = self.current_read_list()
        if rl is None:
            return 0.0
        return 1.0 - self.calc_percentage(rl[: (rl.shape[0] if batch is None else batch)])

    def get_skip_fraction_heads(self, batch: Optional[int] = None) -> Optional[Tensor]:
        """Fraction of tiles the next call skips, per (batch, head): a float32 DEVICE tensor ``(B, H)`` from one launch of
        ``skip_list_stats_heads``, without synchronising (None before the lists exist)."""
        from .flash_attn_interface import skip_list_stats_heads
        rl = self.current_read_list()
        if rl is None:
            return None
        listed = skip_list_stats_heads(rl, batch)
        return 1.0 - listed.to(torch.float32) / float(rl.shape[2] * (rl.shape[3] - 1))

    def snapshot(self) -> dict:
        """Both ping-pong lists, the phase and the step counter, copied ON THE DEVICE (no host round trip, no sync: ``state_dict()``
        takes 112 MB per layer through the host at S = 75 600, H = 40). For ``restore``; thresholds are not part of it."""
        return {"skip_list": None if self._skip_list is None else self._skip_list.clone(), "phase": self._phase, "step": self._step,
                "shape_key": self._shape_key}

    def restore(self, snap: dict):
        """Back to ``snapshot()``: the calls that follow are bit-identical (O, LSE, lists) to those that followed the snapshot. Lists
        of the snapshot's shape are overwritten in place (their addresses stay valid); the snapshot itself is left untouched."""
        if snap["skip_list"] is None:
            self.reset_skip_state()
            return
        if self._skip_list is not None and self._skip_list.shape == snap["skip_list"].shape \
                and self._skip_list.dtype == snap["skip_list"].dtype and self._skip_list.device == snap["skip_list"].device:
            self._skip_list.copy_(snap["skip_list"])
        else:
            self._skip_list = snap["skip_list"].clone()
        self._phase, self._step, self._shape_key = snap["phase"], snap["step"], snap["shape_key"]

    def state_dict(self) -> dict:
        """Everything a run needs to continue bit-identically: both ping-pong lists, the phase, the threshold and what the
        lists were built for (shape key incl. the DEVICE they live on). Tensors are returned on the CPU."""
        key = self._shape_key
        state = {
            "skip_list": None if self._skip_list is None else self._skip_list.detach().cpu().clone(),
            "phase": self._phase, "threshold": self.threshold, "enable_skipping": self.enable_skipping,
            "max_batch_size": self.max_batch_size,
            "shape_key": None if key is None else (*key[:4], str(key[4]).replace("torch.", "")),
            "device": None if key is None else str(key[5]),
            "tile_sizes": None if key is None else tuple(key[6]),
            "list_dtype": str(self.list_dtype).replace("torch.", ""),      # of the saved lists (absent before int16 lists existed: int32)
            "threshold_schedule": None if self._threshold_schedule is None else list(self._threshold_schedule),
            "step": self._step,                                            # both absent before threshold schedules existed: None, 0
        }
        if self._head_thresholds is not None:      # only with a table set: without one the dict is what it was before tables existed
            state["head_thresholds"] = self._head_thresholds.detach().cpu().tolist()      # (H,) or (n_steps, H) as nested lists
        return state

    def load_state_dict(self, state: dict, device=None):
        """Restore ``state_dict()``. The lists are kept in THIS object's ``list_dtype``: a state saved with the other element type is
        converted (widening is exact; narrowing to int16 checks that every value fits and raises ``ValueError`` otherwise). The lists go back to the device they were saved from (``state["device"]``) unless
        ``device`` names another one; a state that records no device (round-1 checkpoints) needs ``device=``. The next call
        must present the same shapes / dtype / device, otherwise the lists are rebuilt as on any shape change (:179-200)."""
        self.threshold = state["threshold"]
        self.enable_skipping = state["enable_skipping"]
        self.max_batch_size = state["max_batch_size"]
        self.reset_skip_state()
        sched = state.get("threshold_schedule")
        self._threshold_schedule = None if sched is None else tuple(float(t) for t in sched)
        table = state.get("head_thresholds")       # the values as they were saved, unchecked: a host table, copied to the device of the next call
        self._set_head_table(None if table is None else torch.tensor(table, dtype=torch.float32))
        if state["skip_list"] is None:
            return
        if device is None:
            device = state.get("device")
            if device is None:
                raise ValueError("this state_dict records no device: pass load_state_dict(state, device=...)")
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())      # query.device always carries an index
        sq, sk, h, d, dt = state["shape_key"]
        dtype = getattr(torch, dt)
        tiles = get_tile_sizes(d, dtype.itemsize)
        saved = state.get("tile_sizes")                       # absent in round-2 checkpoints: the list shape decides
        if saved is not None and tuple(saved) != tuple(tiles):
            raise ValueError(f"this state was saved for kernel tiles {tuple(saved)}, the kernel selected now uses {tuple(tiles)} "
                             "(LA_FWD_KERNEL differs?): the lists cannot be reused")
        if tuple(state["skip_list"].shape[3:]) != (_sl.cdiv(sq, tiles[0]), _sl.cdiv(sk, tiles[1]) + 1):
            raise ValueError("the saved lists do not match the tile geometry of the kernel selected now")
        self._skip_list = _sl.convert_lists(state["skip_list"], self.list_dtype).to(dev).contiguous()
        self._phase = state["phase"]
        self._step = int(state.get("step", 0))
        self._shape_key = (sq, sk, h, d, dtype, dev, tuple(tiles), self.list_dtype)


class SeqParallelLiteAttention:
    """``num_nodes`` independent skip states, one per K/V split, selected by ``split_idx`` (:322-345).
    The (local Q x split j) tile pattern differs per j, hence one state each. Transport of K/V and the
    LSE merge of the partial results stay with the caller; ``flash_attn_combine`` does the merge."""

    def __init__(self, num_nodes: int, enable_skipping: bool = True, threshold: float = -10.0, max_batch_size: int = 4,
                 list_dtype: Optional[torch.dtype] = None):
        self.num_nodes = num_nodes
        self.lite_attention = [LiteAttention(enable_skipping, threshold, max_batch_size, list_dtype) for _ in range(num_nodes)]
        self.set_threshold(threshold)
        # e4m3 inputs with return_softmax_lse=True: the caller merges partial results by that LSE (README.md:222-250), so the split
        # runs with the reference's form of P and its row sums (fp32 sums of the un-rounded P, softmax.h:275-296; fp32-exact LSE) even
        # when the process opted into a faster form (LA_FP8_P / fwd_flags), whose LSE carries the 8-bit rounding of P. Set False to keep
        # whatever form is selected.
        self.exact_fp8_lse = True

    def __call__(self, query: Tensor, key: Tensor, value: Tensor, split_idx: int, scale: Optional[float] = None,
                 return_softmax_lse: bool = False, *, q_descale: Optional[Tensor] = None, k_descale: Optional[Tensor] = None,
                 v_descale: Optional[Tensor] = None, v_shift: Optional[Tensor] = None, lse_shift: Optional[Tensor] = None,
                 out_dtype: Optional[torch.dtype] = None, out_fp8=False) -> Union[Tensor, Tuple[Tensor, Tensor]]:
        """``v_shift`` / ``lse_shift`` / ``out_dtype`` / ``out_fp8`` as ``LiteAttention.__call__``: this shard's output and LSE are
        restored HERE, before the caller merges the shards by LSE - the shards' V means differ, and a merge would weight them.
        (``out_fp8`` is for a shard whose output is final: e4m3 partials are not merged.)"""
        assert split_idx < self.num_nodes, "split_idx must be less than num_nodes"
        kw = {}
        for name, val in (("v_shift", v_shift), ("lse_shift", lse_shift), ("out_dtype", out_dtype)):      # only when given
            if val is not None:
                kw[name] = val
        if out_fp8 is not False:
            kw["out_fp8"] = out_fp8
        if q_descale is not None or k_descale is not None or v_descale is not None:       # keyword-only extension, as LiteAttention.__call__
            kw.update(q_descale=q_descale, k_descale=k_descale, v_descale=v_descale)
        if return_softmax_lse and self.exact_fp8_lse and query.dtype == torch.float8_e4m3fn:
            from .flash_attn_interface import fwd_flags
            from ._cabi import LA_FLAG_FP8_ENCODED_P, LA_FLAG_FP8_MFMA_ROWSUM
            with fwd_flags(0, clear=LA_FLAG_FP8_ENCODED_P | LA_FLAG_FP8_MFMA_ROWSUM):
                return self.lite_attention[split_idx](query, key, value, scale, return_softmax_lse, **kw)
        return self.lite_attention[split_idx](query, key, value, scale, return_softmax_lse, **kw)

    def reset_skip_state(self):
        for la in self.lite_attention:
            la.reset_skip_state()

    def set_threshold(self, threshold: float):
        for la in self.lite_attention:
            la.set_threshold(threshold)

    def set_threshold_schedule(self, thresholds: Optional[Sequence[float]]):
        for la in self.lite_attention:
            la.set_threshold_schedule(thresholds)

    def set_head_thresholds(self, thresholds):
        """``LiteAttention.set_head_thresholds`` on every node: each K/V split votes with the same table."""
        for la in self.lite_attention:
            la.set_head_thresholds(thresholds)

    def enable_skip_optimization(self, enable: bool = True):
        for la in self.lite_attention:
            la.enable_skip_optimization(enable)
