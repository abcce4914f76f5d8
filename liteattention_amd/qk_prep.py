"""The q / k prologue of a Wan2.x-style attention block in one pass over each tensor: RMSNorm, 3-axis RoPE on interleaved pairs and the
cast to bf16 / fp16 (``la_qk_prep``), in place of the ten-odd eager passes with fp32 temporaries that precede the attention call.

    tables = rope_tables((frames, height, width), head_dim, device=x.device)     # once per grid; cached
    q = qk_prep(q_proj.view(b, s, n, d), norm_q.weight, norm_q.eps, tables)      # bf16, ready for LiteAttention
    k = qk_prep(k_proj.view(b, s, n, d), norm_k.weight, norm_k.eps, tables)

``qk_prep_reference`` is the same formula in torch fp64, for tests and for users who want to check.

The e4m3 form (``la_qk_prep_fp8``) is the producer of the fp8 forward's operands: ``qk_prep_fp8`` (scale, clamp, cast to
``float8_e4m3fn`` at the store), ``qk_prep_amax`` (the per-head amax pass alone), ``descale_from_amax`` and ``E4m3Scales``, which keeps
the buffers of one tensor and returns ``(x8, descale)``; the descales then go into the attention call as ``q/k/v_descale``.

K smoothing (``la_qk_prep_smooth``): ``qk_prep_smooth`` subtracts a per-head vector from the keys before it quantizes them and collects
the column sums that vector is made from (``qk_prep_colmean``) and the ``q . c`` row dots that undo its shift of the LSE
(``lse_unshift``); ``SmoothedQK`` keeps the buffers of one layer's q and k.

Row maps (``la_qk_prep_rows`` and its e4m3 and smoothing forms): every call above takes ``rows=`` (out row s is made from row
``rows[s]`` of x) and ``positions=`` (row s is rotated as position ``positions[s]``), so that the attention can run in another token
order than the raster order of the grid; ``token_order.py`` builds the orders."""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import _cabi

_IN_DTYPES = {torch.bfloat16: _cabi.LA_DTYPE_BF16, torch.float16: _cabi.LA_DTYPE_FP16, torch.float32: _cabi.LA_DTYPE_FP32}
_OUT_DTYPES = {torch.bfloat16: _cabi.LA_DTYPE_BF16, torch.float16: _cabi.LA_DTYPE_FP16}
_NORM_MODES = {None: _cabi.LA_NORM_NONE, "none": _cabi.LA_NORM_NONE, "token": _cabi.LA_NORM_TOKEN, "head": _cabi.LA_NORM_HEAD}


class RopeTables(NamedTuple):
    """``tables[a]`` is fp32 ``[grid[a], axis_pairs[a], 2]`` = (cos, sin) of axis a's angles; its first dimension is the axis extent."""
    tables: Tuple[torch.Tensor, torch.Tensor, torch.Tensor]
    axis_pairs: Tuple[int, int, int]


def wan_rope_parts(head_dim: int) -> Tuple[int, int, int]:
    """Elements of a head that each of the (frames, height, width) axes rotates, as Wan splits them: (d - 2 (d // 3), d // 3, d // 3)
    with the last two made even and the first taking the rest."""
    third = head_dim // 3
    third -= third % 2
    return head_dim - 2 * third, third, third


_TABLES = {}      # (grid, head_dim, theta, parts, device) -> RopeTables


def rope_tables(grid: Sequence[int], head_dim: int, theta: float = 10000.0, parts: Optional[Sequence[int]] = None,
                device=None) -> RopeTables:
    """The three (cos, sin) tables ``la_qk_prep`` rotates with, and the pairs per axis. ``grid`` = (e0, e1, e2): token s of a sequence
    sits at (s // (e1 e2), (s // e2) % e1, s % e2). ``parts``: elements of a head per axis (even, their sum at most ``head_dim``; what is
    left passes through unrotated); default ``wan_rope_parts(head_dim)``. 1-D RoPE is ``grid=(S, 1, 1), parts=(head_dim, 0, 0)``.
    Axis a with d elements uses the frequencies 1 / theta^(2 i / d), i < d / 2, in fp32 as the eager rope computes them; the angle
    position x frequency is evaluated in fp64 and rounded to fp32 (which makes it the eager rope's own fp32 product), its cosine and
    sine are evaluated in fp64 and rounded to fp32. Built on the host, cached per (grid, head_dim, theta, parts, device)."""
    grid = tuple(int(g) for g in grid)
    parts = wan_rope_parts(head_dim) if parts is None else tuple(int(p) for p in parts)
    if len(grid) != 3 or any(g <= 0 for g in grid):
        raise ValueError(f"grid must be three positive extents, got {grid}")
    if len(parts) != 3 or any(p < 0 or p % 2 for p in parts) or sum(parts) > head_dim:
        raise ValueError(f"parts must be three even, non-negative element counts summing to at most head_dim = {head_dim}, got {parts}")
    device = torch.device("cpu" if device is None else device)
    key = (grid, int(head_dim), float(theta), parts, str(device))
    hit = _TABLES.get(key)
    if hit is not None:
        return hit
    tables = []
    for extent, d in zip(grid, parts):
        if d == 0:
            tables.append(torch.zeros(extent, 0, 2, dtype=torch.float32, device=device))
            continue
        freqs = 1.0 / theta ** (torch.arange(0, d, 2).float() / d)
        ang = (torch.arange(extent).double()[:, None] * freqs.double()[None]).float().double()
        tables.append(torch.stack((ang.cos(), ang.sin()), dim=-1).float().contiguous().to(device))
    while len(_TABLES) >= 16:                                    # a handful of grids per process; never grow without bound
        _TABLES.pop(next(iter(_TABLES)))
    res = _TABLES[key] = RopeTables(tuple(tables), tuple(p // 2 for p in parts))
    return res


def _unpack_tables(tables, head_dim):
    if tables is None:
        return None, (0, 0, 0)
    tabs, pairs = tables
    pairs = tuple(int(n) for n in pairs)
    if len(tabs) != 3 or len(pairs) != 3:
        raise ValueError("tables: (three tensors, three pair counts), as rope_tables returns them")
    for t, n in zip(tabs, pairs):
        if t.dtype != torch.float32 or t.dim() != 3 or t.shape[1] != n or t.shape[2] != 2 or not t.is_contiguous():
            raise ValueError(f"a rope table must be contiguous fp32 [extent, {n}, 2], got {t.dtype} {tuple(t.shape)}")
    if sum(pairs) > head_dim // 2:
        raise ValueError(f"the axes rotate {sum(pairs)} pairs, a head has {head_dim // 2}")
    return tuple(tabs), pairs


def _check_x(x, reference, name="x", dtypes=_IN_DTYPES, accepted="bf16, fp16 or fp32"):
    """What every prologue pass asks of the (B, S, H, D) tensor it reads; ``reference``: the torch formula the message points to."""
    if x.dim() != 4:
        raise ValueError(f"{name} must be (B, S, H, D), got {tuple(x.shape)}")
    if not x.is_cuda:
        raise ValueError(f"{name} must live on a GPU (there is no CPU path; {reference} is the formula in torch)")
    if x.dtype not in dtypes:
        raise TypeError(f"{name}: {accepted}, got {x.dtype}")


def _check_x_norm(x, norm, reference):
    """``_check_x`` and the norm mode (``la_norm_mode``) of ``norm``."""
    _check_x(x, reference)
    if norm not in _NORM_MODES:
        raise ValueError('norm: "token", "head" or None')
    return _NORM_MODES[norm]


def _check_weight(x, weight, mode):
    if weight is not None and mode != _cabi.LA_NORM_NONE:
        want = x.shape[2] * x.shape[3] if mode == _cabi.LA_NORM_TOKEN else x.shape[3]
        if weight.dtype != torch.float32 or weight.numel() != want or not weight.is_contiguous() or weight.device != x.device:
            raise ValueError(f"weight must be contiguous fp32 with {want} elements on {x.device} "
                             f"(got {weight.dtype}, {tuple(weight.shape)}, {weight.device})")


def _f32(name, t, shape, device):
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or t.device != device:
        raise ValueError(f"{name} must be fp32 {tuple(shape)} on {device}, got {t.dtype} {tuple(t.shape)} on {t.device}")


def _check_scales(x, heads_per_scale, descale, amax):
    """The scale tensors of the e4m3 forms, fp32 (B, H // heads_per_scale) each. Returns heads_per_scale as an int."""
    B, H, hps = x.shape[0], x.shape[2], int(heads_per_scale)
    if hps < 1 or H % hps:
        raise ValueError(f"heads_per_scale must be a divisor of the {H} heads, got {heads_per_scale}")
    for name, t in (("descale", descale), ("amax_out", amax)):
        if t is not None:
            _f32(name, t, (B, H // hps), x.device)
    return hps


def _e4m3_out(x, out, seqlen=None):
    """``out`` of a quantizing pass (allocated when None), checked against ``x`` (``seqlen``: its rows under a row map)."""
    shape = _out_shape(x, x.shape[1] if seqlen is None else seqlen)
    if out is None:
        out = torch.empty(shape, dtype=torch.float8_e4m3fn, device=x.device)
    if out.dtype != torch.float8_e4m3fn:
        raise TypeError(f"out: float8_e4m3fn, got {out.dtype}")
    if tuple(out.shape) != shape or out.device != x.device:
        raise ValueError(f"out must be {shape} on {x.device}, got {tuple(out.shape)} on {out.device}")
    return out


def _map_table(name, t, x, seqlen=None):
    """An int32 table ``[S]`` or ``[B, S]`` on ``x.device`` (or a ``TokenOrder``: its ``src_rows``) -> (table, S, batch stride).
    Metadata only: the entries were checked when the table was built (``TokenOrder.from_rows``), or are the caller's, and the kernel
    clamps them."""
    t = getattr(t, "src_rows", t)
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
        raise TypeError(f"{name}: a TokenOrder or an int32 tensor, got {getattr(t, 'dtype', type(t).__name__)}")
    if t.dim() not in (1, 2) or (t.dim() == 2 and t.shape[0] != x.shape[0]):
        raise ValueError(f"{name} must be [S] or [{x.shape[0]}, S], got {tuple(t.shape)}")
    if t.device != x.device:
        raise ValueError(f"{name} lives on {t.device}, x on {x.device}")
    if t.stride(-1) != 1:
        raise ValueError(f"the last dimension of {name} must be contiguous")
    if seqlen is not None and t.shape[-1] != seqlen:
        raise ValueError(f"{name} has {t.shape[-1]} entries, the result has {seqlen} rows")
    return t, t.shape[-1], (t.stride(0) if t.dim() == 2 and t.shape[0] > 1 else 0)


def _row_map(x, rows, positions):
    """``(la_row_map or None, rows of the result)`` for the ``rows=`` / ``positions=`` of a prologue call on ``x`` (B, S_x, H, D):
    ``rows`` names the row of x each out row is made from (the result has as many rows as the table), ``positions`` the rope position
    of each out row (default: the source row). Checks shapes, dtypes and devices - before anything launches."""
    if rows is None and positions is None:
        return None, x.shape[1]
    m = _cabi.LaRowMap()
    m.struct_size, m.src_seqlen = ctypes.sizeof(_cabi.LaRowMap), x.shape[1]
    seqlen, strides, keep = None, set(), []
    if rows is not None:
        t, seqlen, bs = _map_table("rows", rows, x)
        m.src_rows = t.data_ptr()
        strides.add(bs)
        keep.append(t)
    if positions is not None:
        t, seqlen, bs = _map_table("positions", positions, x, seqlen if rows is not None else x.shape[1])
        m.positions = t.data_ptr()
        strides.add(bs)
        keep.append(t)
    if len(strides) > 1:
        raise ValueError("rows and positions must both be [S] or both be [B, S] with one batch stride")
    m.batch_stride = strides.pop()
    m._keep = keep                                               # the tables live as long as the struct that points at them
    return m, seqlen


def _out_shape(x, seqlen):
    return (x.shape[0], seqlen, x.shape[2], x.shape[3])


def _prep_args(struct, x, out, mode, weight, eps, pos_offset, tables, axis_pairs, seqlen=None):
    """A ``struct`` (one of the three argument structs) with the fields all three share filled in; ``out`` None: nothing is stored.
    ``seqlen``: rows of the result under a row map (default: those of x)."""
    a = struct()
    a.struct_size = ctypes.sizeof(struct)
    a.in_dtype, a.norm_mode = _IN_DTYPES[x.dtype], mode
    a.x = x.data_ptr()
    a.x_batch_stride, a.x_row_stride, a.x_head_stride = x.stride(0), x.stride(1), x.stride(2)
    if out is not None:
        a.out = out.data_ptr()
        a.out_batch_stride, a.out_row_stride, a.out_head_stride = out.stride(0), out.stride(1), out.stride(2)
    a.batch, a.seqlen, a.num_heads, a.head_dim = x.shape
    if seqlen is not None:
        a.seqlen = seqlen
    a.weight = None if weight is None or mode == _cabi.LA_NORM_NONE else weight.data_ptr()
    a.eps, a.pos_offset = float(eps), int(pos_offset)
    if tables is not None:
        for i, (t, n) in enumerate(zip(tables, axis_pairs)):
            if t.device != x.device:
                raise ValueError(f"rope table {i} lives on {t.device}, x on {x.device}: build the tables with device=x.device")
            a.rope_table[i] = t.data_ptr() if n > 0 else None
            a.axis_extent[i], a.axis_pairs[i] = t.shape[0], n
    return a


def _fill_scales(a, hps, descale, amax, store):
    a.heads_per_scale = hps
    if store and descale is not None:
        a.descale, a.descale_batch_stride, a.descale_head_stride = descale.data_ptr(), descale.stride(0), descale.stride(1)
    if amax is not None:
        a.amax, a.amax_batch_stride, a.amax_head_stride = amax.data_ptr(), amax.stride(0), amax.stride(1)


def _call(entry, x, detail, *args):
    """``entry(*args, stream)`` of the library on the device and current stream of ``x``; a status other than LA_OK raises
    ``RuntimeError`` with the status string and ``detail()``."""
    with torch.cuda.device(x.device):
        rc = getattr(_cabi.load(), entry)(*args, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != _cabi.LA_OK:
        raise RuntimeError(f"{entry}: {_cabi.status_string(rc)} ({detail()})")


def _call_prep(entry, a, x, pos_offset, detail, row_map=None):
    """``_call`` of one of the three prologue entry points - its ``_rows`` form when the call has a ``row_map``; ``detail()``: what the
    form adds between the strides of x and the grid."""
    mapped = () if row_map is None else (ctypes.byref(row_map),)
    _call(entry + ("_rows" if mapped else ""), x,
          lambda: f"x {tuple(x.shape)} strides {x.stride()}, {detail()}, pos_offset {pos_offset}, {a.seqlen} rows on a grid "
                  f"of {[int(v) for v in a.axis_extent]}, pairs {[int(v) for v in a.axis_pairs]}"
                  + ("" if row_map is None else f", row map: rows {bool(row_map.src_rows)}, positions {bool(row_map.positions)}, "
                                                f"batch stride {row_map.batch_stride}"), ctypes.byref(a), *mapped)


def _qk_prep_impl(x, weight=None, eps=1e-6, tables=None, axis_pairs=None, norm="token", pos_offset=0, out=None, out_dtype=None,
                  rows=None, positions=None):
    mode = _check_x_norm(x, norm, "qk_prep_reference")
    row_map, seqlen = _row_map(x, rows, positions)
    shape = _out_shape(x, seqlen)
    if out is None:
        if out_dtype is None:
            out_dtype = x.dtype if x.dtype in _OUT_DTYPES else torch.bfloat16
        out = torch.empty(shape, dtype=out_dtype, device=x.device)
    elif out_dtype is not None and out.dtype != out_dtype:
        raise TypeError(f"out is {out.dtype}, out_dtype says {out_dtype}")
    if out.dtype not in _OUT_DTYPES:
        raise TypeError(f"out: bf16 or fp16, got {out.dtype}")
    if tuple(out.shape) != shape or out.device != x.device:
        raise ValueError(f"out must be {shape} on {x.device}, got {tuple(out.shape)} on {out.device}")
    if x.stride(-1) != 1 or out.stride(-1) != 1:
        raise ValueError("the last dimension of x and out must be contiguous")
    if rows is not None and out.data_ptr() == x.data_ptr():
        raise ValueError("rows= gathers: out must not be x (no in-place form)")
    if x.shape[0] * x.shape[1] * seqlen == 0:
        return out
    _check_weight(x, weight, mode)
    a = _prep_args(_cabi.LaQkPrepArgs, x, out, mode, weight, eps, pos_offset, tables, axis_pairs, seqlen)
    a.out_dtype = _OUT_DTYPES[out.dtype]
    _call_prep("la_qk_prep", a, x, pos_offset, lambda: f"out strides {out.stride()}, norm {norm!r}", row_map)
    return out


def qk_prep(x: torch.Tensor, weight: Optional[torch.Tensor] = None, eps: float = 1e-6, tables: Optional[RopeTables] = None,
            norm: Optional[str] = "token", pos_offset: int = 0, out: Optional[torch.Tensor] = None,
            out_dtype: Optional[torch.dtype] = None, *, rows=None, positions=None) -> torch.Tensor:
    """``out = cast(rope(rmsnorm(x) * weight))`` for ``x`` (B, S, H, D) bf16 / fp16 / fp32 on the GPU, in one pass (``la_qk_prep``):
    fp32 arithmetic, one rounding at the store. ``x`` may be any view whose last dimension is contiguous and whose rows start on
    16-byte boundaries - e.g. the q or k slice of a fused (B, S, 3, H, D) projection.

    norm      "token": RMSNorm over the H * D elements of a token (Wan's ``RMSNorm(dim)``; ``weight`` fp32 [H * D]; H * D <= 16384),
              "head": over the D elements of a head (``weight`` fp32 [D]), None: no norm, ``weight`` ignored. ``weight=None``: ones.
    tables    what ``rope_tables`` returns, on ``x.device``; None: no rotation. Row s is rotated as position ``pos_offset + s`` of the
              tables' grid (a chunk of a longer sequence passes its first position).
    out       bf16 or fp16, same shape; default: a new contiguous tensor of ``out_dtype`` (default: ``x.dtype``, bf16 for fp32 input).
              ``out`` may BE ``x`` (same dtype, same strides: in place); any other overlap of the two is an error nobody detects.
    rows      a ``TokenOrder`` or an int32 table ``[S']`` / ``[B, S']`` on ``x.device``: out row s is made from row ``rows[s]`` of x
              and rotated as position ``pos_offset + rows[s]`` - the gather into a token order, fused (``la_qk_prep_rows``). The result
              has S' rows; ``out`` must not be ``x``.
    positions a ``TokenOrder`` or an int32 table ``[S]`` / ``[B, S]``: row s is rotated as position ``pos_offset + positions[s]`` - for
              an ``x`` that already is in another order (gathered once at the model boundary), and with ``rows`` to override the
              position of each gathered row. The kernel clamps what it reads from either table (rows into x, positions into the
              tables' grid); ``TokenOrder.from_rows`` is where a table is checked, once.
    No host sync, no allocation besides ``out``; asynchronous on the current stream. It captures into a HIP graph when the tables
    were built before the capture (building them copies from the host)."""
    tabs, pairs = _unpack_tables(tables, x.shape[-1] if x.dim() else 0)
    return _qk_prep_impl(x, weight, eps, tabs, pairs, norm, pos_offset, out, out_dtype, rows, positions)


def _reference_table(name, t, x):
    """``rows`` / ``positions`` of a reference function as an int64 ``(1 or B, S)`` tensor on ``x.device`` (None stays None)."""
    if t is None:
        return None
    t = getattr(t, "src_rows", t)
    t = torch.as_tensor(t)
    if t.dtype.is_floating_point or t.dim() not in (1, 2) or (t.dim() == 2 and t.shape[0] not in (1, x.shape[0])):
        raise ValueError(f"{name} must be an integer table [S] or [{x.shape[0]}, S], got {t.dtype} {tuple(t.shape)}")
    return (t if t.dim() == 2 else t[None]).to(device=x.device, dtype=torch.int64)


def qk_prep_reference(x: torch.Tensor, weight: Optional[torch.Tensor] = None, eps: float = 1e-6, tables: Optional[RopeTables] = None,
                      norm: Optional[str] = "token", pos_offset: int = 0, out_dtype: Optional[torch.dtype] = None, *, rows=None,
                      positions=None) -> torch.Tensor:
    """The formula of ``qk_prep`` in torch fp64 on whatever device ``x`` lives on, from the same fp32 weight and tables. Returns fp64
    (the unrounded value), or ``out_dtype`` when given. ``rows`` / ``positions``: integer tables ``[S]`` or ``[B, S]`` (or a
    ``TokenOrder``) as in ``qk_prep``; here an entry outside its range raises (the kernel clamps it)."""
    if x.dim() != 4:
        raise ValueError(f"x must be (B, S, H, D), got {tuple(x.shape)}")
    if norm not in _NORM_MODES:
        raise ValueError('norm: "token", "head" or None')
    mode = _NORM_MODES[norm]
    rows, positions = _reference_table("rows", rows, x), _reference_table("positions", positions, x)
    if rows is not None:
        if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= x.shape[1]):
            raise ValueError(f"rows has an entry outside [0, {x.shape[1]})")
        x = torch.stack([x[b, rows[b if rows.shape[0] > 1 else 0]] for b in range(x.shape[0])])
        if positions is None:
            positions = rows
    B, S, H, D = x.shape
    if positions is not None and positions.shape[1] != S:
        raise ValueError(f"positions has {positions.shape[1]} entries, the result has {S} rows")
    y = x.double()
    if mode != _cabi.LA_NORM_NONE:
        eps64 = float(torch.tensor(eps, dtype=torch.float32))                 # the kernel is handed eps as fp32
        dims = (2, 3) if mode == _cabi.LA_NORM_TOKEN else (3,)
        y = y * torch.rsqrt(y.pow(2).mean(dims, keepdim=True) + eps64)
        if weight is not None:
            y = y * (weight.double().view(H, D) if mode == _cabi.LA_NORM_TOKEN else weight.double().view(D))
    tabs, pairs = _unpack_tables(tables, D)
    if tabs is not None and sum(pairs) > 0:
        e1, e2 = tabs[1].shape[0], tabs[2].shape[0]
        pos = pos_offset + (torch.arange(S, device=x.device)[None] if positions is None else positions)      # (1 or B, S)
        if pos_offset < 0 or (pos.numel() and (int(pos.min()) < 0 or int(pos.max()) >= tabs[0].shape[0] * e1 * e2)):
            raise ValueError("pos_offset + S exceeds the grid of the tables" if positions is None else
                             "pos_offset + positions leaves the grid of the tables")
        coords = (pos // (e1 * e2), (pos // e2) % e1, pos % e2)
        cs = torch.cat([t.to(x.device)[c].double() for t, c in zip(tabs, coords)], dim=2)      # (1 or B, S, rotated pairs, 2)
        n = cs.shape[2]
        cos, sin = cs[:, :, None, :, 0], cs[:, :, None, :, 1]
        pair = y[..., :2 * n].reshape(B, S, H, n, 2)
        a, b = pair[..., 0], pair[..., 1]
        rot = torch.stack((a * cos - b * sin, a * sin + b * cos), dim=-1).reshape(B, S, H, 2 * n)
        y = torch.cat((rot, y[..., 2 * n:]), dim=-1)
    return y if out_dtype is None else y.to(out_dtype)


# ---- the e4m3 form: la_qk_prep_fp8 -----------------------------------------------------------------------------------------------------------
E4M3_MAX = 448.0
_TINY = 2.0 ** -100        # the smallest amax a descale is made from: its reciprocal, 448 / tiny / margin, stays finite in fp32 (0 * it = 0)


def _qk_prep_fp8_impl(x, weight, eps, tables, axis_pairs, norm, pos_offset, descale, amax, heads_per_scale, out, store, rows=None,
                      positions=None):
    """One ``la_qk_prep_fp8`` call. ``store``: quantize into ``out`` (allocated when None); otherwise the amax pass alone."""
    mode = _check_x_norm(x, norm, "qk_prep_fp8_reference")
    hps = _check_scales(x, heads_per_scale, descale, amax)
    row_map, seqlen = _row_map(x, rows, positions)
    if store:
        out = _e4m3_out(x, out, seqlen)
    elif amax is None:
        raise ValueError("the amax pass needs amax_out")
    if x.stride(-1) != 1 or (store and out.stride(-1) != 1):
        raise ValueError("the last dimension of x and out must be contiguous")
    if x.shape[0] * x.shape[1] * seqlen == 0:
        return out
    _check_weight(x, weight, mode)
    a = _prep_args(_cabi.LaQkPrepFp8Args, x, out if store else None, mode, weight, eps, pos_offset, tables, axis_pairs, seqlen)
    _fill_scales(a, hps, descale, amax, store)
    _call_prep("la_qk_prep_fp8", a, x, pos_offset,
               lambda: f"out strides {out.stride() if store else None}, norm {norm!r}, heads_per_scale {hps}", row_map)
    return out


def qk_prep_fp8(x: torch.Tensor, weight: Optional[torch.Tensor] = None, eps: float = 1e-6, tables: Optional[RopeTables] = None,
                norm: Optional[str] = "token", pos_offset: int = 0, *, descale: Optional[torch.Tensor] = None,
                amax_out: Optional[torch.Tensor] = None, heads_per_scale: int = 1, out: Optional[torch.Tensor] = None,
                rows=None, positions=None) -> torch.Tensor:
    """``qk_prep`` with a ``float8_e4m3fn`` result (``la_qk_prep_fp8``): with y the fp32 value ``qk_prep`` would round,
    ``out = e4m3(clamp(y / descale[b, h // heads_per_scale], -448, 448))``, round to nearest even, a NaN stays a NaN.

    descale          fp32 (B, H // heads_per_scale), the tensor the attention call then takes as ``q_descale`` / ``k_descale`` /
                     ``v_descale`` (``heads_per_scale`` = 1 for k and v, H_q // H_kv for q); None: 1.0. A descale that is zero, negative
                     or not finite is the caller's error.
    amax_out         fp32 (B, H // heads_per_scale): raised to the largest ``|y|`` of its group (a RUNNING maximum: zero it for a fresh
                     one; a NaN in the group makes it NaN). None: not computed.
    norm / tables    as ``qk_prep``; ``norm=None`` without tables is the V form (scale, clamp, cast, amax).
    out              float8_e4m3fn, same shape, rows / heads / batches on 8-byte boundaries; it must not overlap ``x``.
    rows / positions as ``qk_prep`` (``la_qk_prep_fp8_rows``): a row's bytes depend on its source row and its position alone, the amax
                     on no order at all.
    No host sync, no allocation besides ``out``; asynchronous on the current stream; captures into a HIP graph like ``qk_prep``."""
    tabs, pairs = _unpack_tables(tables, x.shape[-1] if x.dim() else 0)
    return _qk_prep_fp8_impl(x, weight, eps, tabs, pairs, norm, pos_offset, descale, amax_out, heads_per_scale, out, True, rows, positions)


def qk_prep_amax(x: torch.Tensor, weight: Optional[torch.Tensor] = None, eps: float = 1e-6, tables: Optional[RopeTables] = None,
                 norm: Optional[str] = "token", pos_offset: int = 0, *, amax_out: Optional[torch.Tensor] = None,
                 heads_per_scale: int = 1, rows=None, positions=None) -> torch.Tensor:
    """The amax pass of ``qk_prep_fp8`` alone: x is read once, nothing else is written. Returns ``amax_out`` (B, H // heads_per_scale)
    fp32 raised to the largest ``|y|`` of each group - the bits the quantizing call reports; None: a new zeroed tensor.
    ``rows`` / ``positions``: as ``qk_prep_fp8`` (the maximum is taken over the rows the map names)."""
    tabs, pairs = _unpack_tables(tables, x.shape[-1] if x.dim() else 0)
    if amax_out is None and x.dim() == 4:
        amax_out = torch.zeros((x.shape[0], x.shape[2] // max(1, int(heads_per_scale))), dtype=torch.float32, device=x.device)
    _qk_prep_fp8_impl(x, weight, eps, tabs, pairs, norm, pos_offset, None, amax_out, heads_per_scale, None, False, rows, positions)
    return amax_out


def descale_from_amax(amax: torch.Tensor, margin: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``clamp_min(amax, tiny) * margin / 448``: the descale under which the largest ``|y|`` seen lands on ``448 / margin``. On the
    device of ``amax``, no host sync, graph-capturable; a NaN amax gives a NaN descale (and NaN outputs: the signal survives)."""
    out = torch.clamp_min(amax, _TINY, out=out)
    return out.mul_(float(margin)).div_(E4M3_MAX)


def qk_prep_fp8_reference(x: torch.Tensor, weight: Optional[torch.Tensor] = None, eps: float = 1e-6, tables: Optional[RopeTables] = None,
                          norm: Optional[str] = "token", pos_offset: int = 0, *, descale: Optional[torch.Tensor] = None,
                          heads_per_scale: int = 1, rows=None, positions=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The formula of ``qk_prep_fp8`` in torch fp64: ``(clamp(y / descale, -448, 448)`` UNROUNDED, ``amax`` (B, H // heads_per_scale)
    of the unscaled ``|y|)``, both fp64, with ``y = qk_prep_reference(...)`` (``rows`` / ``positions`` included)."""
    y = qk_prep_reference(x, weight, eps, tables, norm, pos_offset, rows=rows, positions=positions)
    B, S, H, D = y.shape
    hps = int(heads_per_scale)
    if hps < 1 or H % hps:
        raise ValueError(f"heads_per_scale must be a divisor of the {H} heads, got {heads_per_scale}")
    amax = y.abs().reshape(B, S, H // hps, hps * D).amax(dim=(1, 3))          # (amax propagates a NaN, as the kernel's does)
    if descale is not None:
        y = y / descale.double().to(y.device).repeat_interleave(hps, dim=1)[:, None, :, None]
    return y.clamp(-E4M3_MAX, E4M3_MAX), amax


class E4m3Scales:
    """The amax and descale buffers of ONE tensor (q, k or v of one layer) across calls: ``x8, descale = scales(x, ...)`` quantizes
    with ``qk_prep_fp8`` and returns the descale to hand to the attention call.

    mode "current"   every call runs the amax pass, makes the descale from it and quantizes with it: exact, two reads of x.
    mode "delayed"   step t quantizes with the descale made from step t - 1's amax and collects its own amax in the same pass: one
                     read of x. The first call has no history and runs the amax pass. ``margin`` > 1 leaves headroom for the growth
                     of amax from one step to the next (what exceeds it saturates at +-448).
    tiles=True       for a V only the attention call reads (``norm=None``, no weight, no tables, ``heads_per_scale`` 1): the quantizing
                     pass is ``v_prep.v_prep_tiles`` and ``x8`` a ``PreparedV`` - the V^T tiles of the e4m3 forward, no e4m3 tensor.
    The buffers (amax, descale, the e4m3 result) are allocated by the first call and reused: no host sync, no allocation after
    it - the result of a call is overwritten by the next one."""

    _amax_pass = staticmethod(qk_prep_amax)
    _quant_pass = staticmethod(qk_prep_fp8)

    def __init__(self, mode: str = "current", margin: float = 1.0, heads_per_scale: int = 1, tiles: bool = False):
        if mode not in ("current", "delayed"):
            raise ValueError('mode: "current" or "delayed"')
        if not margin > 0:
            raise ValueError("margin must be positive")
        if tiles and int(heads_per_scale) != 1:
            raise ValueError("tiles=True takes one descale per kv head (heads_per_scale 1), as the attention call does")
        self.mode, self.margin, self.heads_per_scale, self.tiles = mode, float(margin), int(heads_per_scale), bool(tiles)
        self.amax = self.descale = self.out = None
        self.calls = 0

    def __call__(self, x, weight=None, eps=1e-6, tables=None, norm="token", pos_offset=0, *, rows=None, positions=None):
        """``rows`` / ``positions``: as ``qk_prep_fp8``, for both passes. ``tiles=True`` takes no map: gather V first
        (``TokenOrder.gather``)."""
        B, S, H, D = x.shape
        hps = self.heads_per_scale
        mapped = dict(rows=rows, positions=positions) if rows is not None or positions is not None else {}
        if mapped:
            S = _row_map(x, rows, positions)[1]
        if self.tiles:
            from . import v_prep                                     # (v_prep imports this module)
            if norm is not None or weight is not None or tables is not None:
                raise ValueError("tiles=True quantizes V as its projection wrote it: norm=None, no weight, no tables")
            if mapped:
                raise ValueError("tiles=True (v_prep_tiles) takes no row map: bring V into the order first with TokenOrder.gather")
        first = self.amax is None or tuple(self.out.shape) != (B, S, H, D) or self.out.device != x.device
        if first:
            self.amax = torch.zeros((B, H // hps), dtype=torch.float32, device=x.device)
            self.descale = torch.empty_like(self.amax)
            if self.tiles:
                self.out = v_prep.PreparedV(torch.empty(v_prep.v_tiles_bytes(B, H, S, D)[1], dtype=torch.uint8, device=x.device),
                                            x.shape, self.descale)
            else:
                self.out = torch.empty((B, S, H, D), dtype=torch.float8_e4m3fn, device=x.device)
        if first or self.mode == "current":
            self.amax.zero_()
            self._amax_pass(x, weight, eps, tables, norm, pos_offset, amax_out=self.amax, heads_per_scale=hps, **mapped)
        descale_from_amax(self.amax, self.margin, out=self.descale)
        collect = None
        if self.mode == "delayed":                               # this step's amax, for the next step's descale
            self.amax.zero_()
            collect = self.amax
        if self.tiles:
            v_prep.v_prep_tiles(x, descale=self.descale, amax_out=collect, out=self.out)
        else:
            self._quant_pass(x, weight, eps, tables, norm, pos_offset, descale=self.descale, amax_out=collect, heads_per_scale=hps,
                             out=self.out, **mapped)
        self.calls += 1
        return self.out, self.descale


# ---- K smoothing: la_qk_prep_smooth ----------------------------------------------------------------------------------------------------------
def qk_prep_smooth_parts(seqlen: int, num_heads: int, head_dim: int) -> Tuple[int, int]:
    """``(n_parts, rows_per_part)`` of the column partial sums of ``qk_prep_smooth`` for a shape (``la_qk_prep_smooth_parts`` and
    ``la_qk_prep_smooth_part_rows``): part p holds rows ``[p * rows_per_part, (p + 1) * rows_per_part)`` of each batch."""
    lib = _cabi.load()
    n = lib.la_qk_prep_smooth_parts(int(seqlen), int(num_heads), int(head_dim))
    r = lib.la_qk_prep_smooth_part_rows(int(seqlen), int(num_heads), int(head_dim))
    if n <= 0 or r <= 0:
        raise ValueError(f"la_qk_prep_smooth_parts({seqlen}, {num_heads}, {head_dim}): {_cabi.status_string(min(n, r))}")
    return n, r


def _qk_prep_smooth_impl(x, weight, eps, tables, axis_pairs, norm, pos_offset, shift, descale, amax, heads_per_scale, colsum_part,
                         dot_vec, heads_per_dot, dot_out, out, store, rows=None, positions=None):
    """One ``la_qk_prep_smooth`` call. ``store``: quantize into ``out`` (allocated when None)."""
    mode = _check_x_norm(x, norm, "qk_prep_smooth_reference")
    B, _, H, D = x.shape
    row_map, S = _row_map(x, rows, positions)                    # S: rows of the result - of out, of dot_out and of the parts
    hps, hpd = _check_scales(x, heads_per_scale, descale, amax), int(heads_per_dot)
    if shift is not None:
        _f32("shift", shift, (B, H, D), x.device)
        if shift.stride(2) != 1:
            raise ValueError("the last dimension of shift must be contiguous")
    if dot_vec is not None:
        if hpd < 1 or H % hpd:
            raise ValueError(f"heads_per_dot must be a divisor of the {H} heads, got {heads_per_dot}")
        _f32("dot_vec", dot_vec, (B, H // hpd, D), x.device)
        if dot_vec.stride(2) != 1:
            raise ValueError("the last dimension of dot_vec must be contiguous")
        if dot_out is None:
            dot_out = torch.empty((B, H, S), dtype=torch.float32, device=x.device)
        _f32("dot_out", dot_out, (B, H, S), x.device)
        if not dot_out.is_contiguous():
            raise ValueError("dot_out must be contiguous")
    elif dot_out is not None:
        raise ValueError("dot_out needs dot_vec")
    if B * S * x.shape[1] == 0:
        return out
    if colsum_part is not None:
        n_parts, _ = qk_prep_smooth_parts(S, H, D)
        _f32("colsum_part", colsum_part, (n_parts, B, H, D), x.device)
        if not colsum_part.is_contiguous():
            raise ValueError("colsum_part must be contiguous")
    if store:
        out = _e4m3_out(x, out, S)
    elif amax is None and colsum_part is None and dot_out is None:
        raise ValueError("a pass that stores nothing needs amax_out, colsum_part or dot_vec")
    if x.stride(-1) != 1 or (store and out.stride(-1) != 1):
        raise ValueError("the last dimension of x and out must be contiguous")
    _check_weight(x, weight, mode)
    a = _prep_args(_cabi.LaQkPrepSmoothArgs, x, out if store else None, mode, weight, eps, pos_offset, tables, axis_pairs, S)
    _fill_scales(a, hps, descale, amax, store)
    a.heads_per_dot = hpd
    if shift is not None:
        a.shift, a.shift_batch_stride, a.shift_head_stride = shift.data_ptr(), shift.stride(0), shift.stride(1)
    if colsum_part is not None:
        a.colsum_part = colsum_part.data_ptr()
    if dot_vec is not None:
        a.dot_vec, a.dot_vec_batch_stride, a.dot_vec_head_stride = dot_vec.data_ptr(), dot_vec.stride(0), dot_vec.stride(1)
        a.dot_out = dot_out.data_ptr()
    _call_prep("la_qk_prep_smooth", a, x, pos_offset,
               lambda: f"out strides {out.stride() if store else None}, norm {norm!r}, heads_per_scale {hps}, heads_per_dot {hpd}, shift "
                       f"{None if shift is None else shift.stride()}, part sums {colsum_part is not None}", row_map)
    return out


def qk_prep_smooth(x: torch.Tensor, weight: Optional[torch.Tensor] = None, eps: float = 1e-6, tables: Optional[RopeTables] = None,
                   norm: Optional[str] = "token", pos_offset: int = 0, *, shift: Optional[torch.Tensor] = None,
                   descale: Optional[torch.Tensor] = None, amax_out: Optional[torch.Tensor] = None, heads_per_scale: int = 1,
                   colsum_part: Optional[torch.Tensor] = None, dot_vec: Optional[torch.Tensor] = None, heads_per_dot: int = 1,
                   dot_out: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                   quantize: bool = True, rows=None, positions=None) -> Optional[torch.Tensor]:
    """``qk_prep_fp8`` with K smoothing (``la_qk_prep_smooth``). With y the fp32 value ``qk_prep`` would round:

    shift         fp32 (B, H, D): ``out`` and ``amax_out`` are taken from ``y - shift[b, h]``. Subtracting one vector from every key
                  of a head changes neither P nor O nor the skip vote; the LSE moves by ``-softmax_scale * (q . shift)``.
    colsum_part   fp32 (n_parts, B, H, D) contiguous, ``n_parts`` from ``qk_prep_smooth_parts``: the sums of the UNSHIFTED y over the
                  rows of each part, bit-reproducible (``colsum_finish`` makes the mean of them).
    dot_vec       fp32 (B, H // heads_per_dot, D): ``dot_out[b, h, s] = sum_d y[b, s, h, d] * dot_vec[b, h // heads_per_dot, d]`` of the
                  unshifted, unquantized y, fp32 (B, H, S) - the layout of the LSE. For q, ``dot_vec`` is the shift given for k and
                  ``heads_per_dot`` = H_q // H_kv; ``lse_unshift`` then restores the LSE. ``dot_out`` None: allocated; read it from
                  the ``dot_out`` you pass.
    quantize      False: nothing is stored (a sums-only, dots-only or amax-only pass), returns None.
    rows / positions   as ``qk_prep`` (``la_qk_prep_smooth_rows``): ``out`` and ``dot_out`` are indexed by the row of the RESULT, and the
                  parts of ``colsum_part`` are cut from the rows of the result - the same S terms per column as the unmapped call, added
                  in another order.
    Everything else as ``qk_prep_fp8``; with ``shift``, ``colsum_part`` and ``dot_vec`` all None it is ``qk_prep_fp8``, bit for bit."""
    tabs, pairs = _unpack_tables(tables, x.shape[-1] if x.dim() else 0)
    if not quantize and out is not None:
        raise ValueError("quantize=False stores nothing: out must be None")
    return _qk_prep_smooth_impl(x, weight, eps, tabs, pairs, norm, pos_offset, shift, descale, amax_out, heads_per_scale, colsum_part,
                                dot_vec, heads_per_dot, dot_out, out, bool(quantize), rows, positions)


def colsum_finish(colsum_part: torch.Tensor, seqlen: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``mean[b, h, d] = (part[0, b, h, d] + part[1, b, h, d] + ...) / seqlen``, added in index order (``la_colsum_finish``)."""
    if colsum_part.dim() != 4 or colsum_part.dtype != torch.float32 or not colsum_part.is_contiguous() or not colsum_part.is_cuda:
        raise ValueError("colsum_part must be contiguous fp32 (n_parts, B, H, D) on a GPU")
    n_parts, B, H, D = colsum_part.shape
    if out is None:
        out = torch.empty((B, H, D), dtype=torch.float32, device=colsum_part.device)
    _f32("out", out, (B, H, D), colsum_part.device)
    if out.stride(2) != 1:
        raise ValueError("the last dimension of out must be contiguous")
    _call("la_colsum_finish", colsum_part, lambda: f"parts {tuple(colsum_part.shape)}, seqlen {seqlen}", colsum_part.data_ptr(), n_parts, B, H,
          D, int(seqlen), out.data_ptr(), out.stride(0), out.stride(1))
    return out


def qk_prep_colmean(x: torch.Tensor, weight: Optional[torch.Tensor] = None, eps: float = 1e-6, tables: Optional[RopeTables] = None,
                    norm: Optional[str] = "token", pos_offset: int = 0, *, colsum_part: Optional[torch.Tensor] = None,
                    out: Optional[torch.Tensor] = None, rows=None, positions=None) -> torch.Tensor:
    """The mean of y over the rows, fp32 (B, H, D): the sums-only pass of ``qk_prep_smooth`` plus ``colsum_finish``. x is read once and
    nothing of its size is written. ``colsum_part`` / ``out``: buffers to reuse (None: allocated). ``rows`` / ``positions``: as
    ``qk_prep_smooth`` (the mean over the rows the map names)."""
    _check_x(x, "qk_prep_smooth_reference")
    B, _, H, D = x.shape
    S = _row_map(x, rows, positions)[1]
    if colsum_part is None:
        colsum_part = torch.empty((qk_prep_smooth_parts(S, H, D)[0], B, H, D), dtype=torch.float32, device=x.device)
    qk_prep_smooth(x, weight, eps, tables, norm, pos_offset, colsum_part=colsum_part, quantize=False, rows=rows, positions=positions)
    return colsum_finish(colsum_part, S, out=out)


def qk_prep_smooth_reference(x: torch.Tensor, weight: Optional[torch.Tensor] = None, eps: float = 1e-6,
                             tables: Optional[RopeTables] = None, norm: Optional[str] = "token", pos_offset: int = 0, *,
                             shift: Optional[torch.Tensor] = None, descale: Optional[torch.Tensor] = None, heads_per_scale: int = 1,
                             dot_vec: Optional[torch.Tensor] = None, heads_per_dot: int = 1, rows=None, positions=None):
    """The formula of ``qk_prep_smooth`` in torch fp64, with ``y = qk_prep_reference(...)``: ``(clamp((y - shift) / descale, -448, 448)``
    UNROUNDED, the amax (B, H // heads_per_scale) of ``|y - shift|``, the mean (B, H, D) of y over the rows, the row dots (B, H, S) of y
    with ``dot_vec`` or None``)``, all fp64. ``rows`` / ``positions``: as ``qk_prep_reference``; S is the number of rows of the result."""
    y = qk_prep_reference(x, weight, eps, tables, norm, pos_offset, rows=rows, positions=positions)
    B, S, H, D = y.shape
    hps, hpd = int(heads_per_scale), int(heads_per_dot)
    if hps < 1 or H % hps:
        raise ValueError(f"heads_per_scale must be a divisor of the {H} heads, got {heads_per_scale}")
    mean = y.mean(dim=1)
    dots = None
    if dot_vec is not None:
        if hpd < 1 or H % hpd:
            raise ValueError(f"heads_per_dot must be a divisor of the {H} heads, got {heads_per_dot}")
        dots = torch.einsum("bshd,bhd->bhs", y, dot_vec.double().to(y.device).repeat_interleave(hpd, dim=1))
    z = y if shift is None else y - shift.double().to(y.device)[:, None]
    amax = z.abs().reshape(B, S, H // hps, hps * D).amax(dim=(1, 3))
    if descale is not None:
        z = z / descale.double().to(y.device).repeat_interleave(hps, dim=1)[:, None, :, None]
    return z.clamp(-E4M3_MAX, E4M3_MAX), amax, mean, dots


def lse_unshift(lse: torch.Tensor, dot: torch.Tensor, softmax_scale: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``lse + softmax_scale * dot``: the LSE of the unshifted keys from the LSE the attention call returned for keys shifted by c and
    ``dot`` = q . c (``qk_prep_smooth(..., dot_vec=c)`` on the q side), both (B, H, S) fp32. ``softmax_scale`` is the one given to the
    attention call (its default is ``head_dim ** -0.5``). One torch add: no host sync, captures into a HIP graph. Needed wherever the
    LSE is used - e.g. the merge of the text + video recipe; O needs nothing."""
    return torch.add(lse, dot, alpha=float(softmax_scale), out=out)


class SmoothedQK:
    """The buffers of one layer's q and k across calls, with the keys mean-shifted before they are quantized:
    ``q8, k8, dq, dk, lse_shift = smoothed.pair(xq, xk, wq, wk, eps, tables, norm)``. ``q8, k8`` e4m3, ``dq, dk`` the descales for the
    attention call, ``lse_shift`` (B, H_q, S) = q . c for ``lse_unshift`` (O needs no correction). k is prepared BEFORE q: q's dots need
    the shift k used. V: ``E4m3Scales``, or ``SmoothedV`` (v_prep.py).

    mode "current"   k: the column-mean pass, the amax pass of ``y - mean``, the quantizing pass (three reads of xk);
                     q: the amax pass, the quantizing pass with the dots (two reads of xq).
    mode "delayed"   one read of each tensor: step t shifts by step t - 1's mean and scales by step t - 1's amaxes, and collects its own
                     part sums and amaxes in the same pass; the finish kernel then makes the mean for step t + 1. ANY shift vector is
                     exact, so a stale mean costs no correctness - only the amax may outgrow ``margin``. The first call has no
                     history and runs as "current".
    Buffers are allocated by the first call and reused: no host sync, no allocation after it; a call overwrites the last results."""

    def __init__(self, mode: str = "current", margin: float = 1.0, heads_per_scale: Optional[int] = None):
        if mode not in ("current", "delayed"):
            raise ValueError('mode: "current" or "delayed"')
        if not margin > 0:
            raise ValueError("margin must be positive")
        self.mode, self.margin, self.heads_per_scale = mode, float(margin), heads_per_scale
        self.q8 = self.k8 = None
        self.calls = 0

    def _allocate(self, xq, xk, hps, sq, sk):
        dev = xk.device
        B, _, Hk, D = xk.shape
        S, Hq = sk, xq.shape[2]
        f32 = dict(dtype=torch.float32, device=dev)
        self.q8 = torch.empty(_out_shape(xq, sq), dtype=torch.float8_e4m3fn, device=dev)
        self.k8 = torch.empty(_out_shape(xk, sk), dtype=torch.float8_e4m3fn, device=dev)
        self.amax_q, self.amax_k = torch.zeros((B, Hq // hps), **f32), torch.zeros((B, Hk), **f32)
        self.dq, self.dk = torch.empty_like(self.amax_q), torch.empty_like(self.amax_k)
        self.part = torch.empty((qk_prep_smooth_parts(S, Hk, D)[0], B, Hk, D), **f32)
        self.mean = torch.empty((B, Hk, D), **f32)
        self.lse_shift = torch.empty((B, Hq, sq), **f32)

    def pair(self, xq, xk, wq=None, wk=None, eps=1e-6, tables=None, norm="token", pos_offset=0, *, rows=None, positions=None):
        """``rows`` / ``positions``: one map for q and k (self-attention: both in the same order), as ``qk_prep_smooth``."""
        Hq, Hk = xq.shape[2], xk.shape[2]
        if Hq % Hk:
            raise ValueError(f"{Hq} query heads are no multiple of {Hk} key heads")
        hps = Hq // Hk if self.heads_per_scale is None else int(self.heads_per_scale)
        if hps != Hq // Hk:
            raise ValueError(f"heads_per_scale of q must be H_q // H_kv = {Hq // Hk} (the attention call takes descales per kv head)")
        m = dict(rows=rows, positions=positions)
        sq, sk = _row_map(xq, rows, positions)[1], _row_map(xk, rows, positions)[1]
        first = (self.q8 is None or tuple(self.q8.shape) != _out_shape(xq, sq) or tuple(self.k8.shape) != _out_shape(xk, sk)
                 or self.k8.device != xk.device)
        if first:
            self._allocate(xq, xk, hps, sq, sk)
        args_q, args_k = (xq, wq, eps, tables, norm, pos_offset), (xk, wk, eps, tables, norm, pos_offset)
        if first or self.mode == "current":
            qk_prep_colmean(*args_k, colsum_part=self.part, out=self.mean, **m)
            self.amax_k.zero_()
            qk_prep_smooth(*args_k, shift=self.mean, amax_out=self.amax_k, quantize=False, **m)
            descale_from_amax(self.amax_k, self.margin, out=self.dk)
            qk_prep_smooth(*args_k, shift=self.mean, descale=self.dk, out=self.k8, **m)
            self.amax_q.zero_()
            qk_prep_amax(*args_q, amax_out=self.amax_q, heads_per_scale=hps, **m)
            descale_from_amax(self.amax_q, self.margin, out=self.dq)
            qk_prep_smooth(*args_q, descale=self.dq, heads_per_scale=hps, dot_vec=self.mean, heads_per_dot=hps, dot_out=self.lse_shift,
                           out=self.q8, **m)
        else:
            descale_from_amax(self.amax_k, self.margin, out=self.dk)
            descale_from_amax(self.amax_q, self.margin, out=self.dq)
            self.amax_k.zero_()
            self.amax_q.zero_()
            qk_prep_smooth(*args_k, shift=self.mean, descale=self.dk, amax_out=self.amax_k, colsum_part=self.part, out=self.k8, **m)
            qk_prep_smooth(*args_q, descale=self.dq, amax_out=self.amax_q, heads_per_scale=hps, dot_vec=self.mean, heads_per_dot=hps,
                           dot_out=self.lse_shift, out=self.q8, **m)
            colsum_finish(self.part, sk, out=self.mean)                   # behind q's read of the mean this step used
        self.calls += 1
        return self.q8, self.k8, self.dq, self.dk, self.lse_shift


# ---- op registration: torch.ops.lite_attention.qk_prep, beside fwd / fwd_combine ---------------------------------------------------------
_QK_PREP_SCHEMA = ("qk_prep(Tensor x, Tensor? weight = None, float eps = 1e-6, Tensor[]? tables = None, int[]? axis_pairs = None, "
                   "str? norm = \"token\", int pos_offset = 0, Tensor(out!)? out = None, ScalarType? out_dtype = None) -> Tensor(out!)")
_op_lib = None


def _qk_prep_op(x, weight=None, eps=1e-6, tables=None, axis_pairs=None, norm="token", pos_offset=0, out=None, out_dtype=None):
    tabs, pairs = _unpack_tables(None if tables is None else (tables, axis_pairs or ()), x.shape[-1])
    return _qk_prep_impl(x, weight, eps, tabs, pairs, norm, pos_offset, out, out_dtype)


def _qk_prep_meta(x, weight=None, eps=1e-6, tables=None, axis_pairs=None, norm="token", pos_offset=0, out=None, out_dtype=None):
    """Shapes and dtypes only (fake-tensor tracing treats the op as opaque)."""
    if out is not None:
        return out
    if out_dtype is None:
        out_dtype = x.dtype if x.dtype in _OUT_DTYPES else torch.bfloat16
    return torch.empty(x.shape, dtype=out_dtype, device=x.device)


_QK_PREP_FP8_SCHEMA = ("qk_prep_fp8(Tensor x, Tensor? weight = None, float eps = 1e-6, Tensor[]? tables = None, int[]? axis_pairs = None, "
                       "str? norm = \"token\", int pos_offset = 0, Tensor? descale = None, Tensor(amax!)? amax_out = None, "
                       "int heads_per_scale = 1, Tensor(out!)? out = None) -> Tensor(out!)")


def _qk_prep_fp8_op(x, weight=None, eps=1e-6, tables=None, axis_pairs=None, norm="token", pos_offset=0, descale=None, amax_out=None,
                    heads_per_scale=1, out=None):
    tabs, pairs = _unpack_tables(None if tables is None else (tables, axis_pairs or ()), x.shape[-1])
    return _qk_prep_fp8_impl(x, weight, eps, tabs, pairs, norm, pos_offset, descale, amax_out, heads_per_scale, out, True)


def _e4m3_meta(x, out):
    """Shape and dtype only, of the two e4m3 ops."""
    return out if out is not None else torch.empty(x.shape, dtype=torch.float8_e4m3fn, device=x.device)


def _qk_prep_fp8_meta(x, weight=None, eps=1e-6, tables=None, axis_pairs=None, norm="token", pos_offset=0, descale=None, amax_out=None,
                      heads_per_scale=1, out=None):
    return _e4m3_meta(x, out)      # (named arguments: the dispatcher drops trailing arguments that equal their defaults)


_QK_PREP_SMOOTH_SCHEMA = ("qk_prep_smooth(Tensor x, Tensor? weight = None, float eps = 1e-6, Tensor[]? tables = None, "
                          "int[]? axis_pairs = None, str? norm = \"token\", int pos_offset = 0, Tensor? shift = None, Tensor? descale = None, "
                          "Tensor(amax!)? amax_out = None, int heads_per_scale = 1, Tensor(part!)? colsum_part = None, "
                          "Tensor? dot_vec = None, int heads_per_dot = 1, Tensor(dots!)? dot_out = None, Tensor(out!)? out = None) "
                          "-> Tensor(out!)")


def _qk_prep_smooth_op(x, weight=None, eps=1e-6, tables=None, axis_pairs=None, norm="token", pos_offset=0, shift=None, descale=None,
                       amax_out=None, heads_per_scale=1, colsum_part=None, dot_vec=None, heads_per_dot=1, dot_out=None, out=None):
    """The quantizing form (the op returns a tensor); with ``dot_vec`` it wants ``dot_out`` too."""
    tabs, pairs = _unpack_tables(None if tables is None else (tables, axis_pairs or ()), x.shape[-1])
    if dot_vec is not None and dot_out is None:
        raise ValueError("the op writes the dots into dot_out: give it")
    return _qk_prep_smooth_impl(x, weight, eps, tabs, pairs, norm, pos_offset, shift, descale, amax_out, heads_per_scale, colsum_part,
                                dot_vec, heads_per_dot, dot_out, out, True)


def _qk_prep_smooth_meta(x, weight=None, eps=1e-6, tables=None, axis_pairs=None, norm="token", pos_offset=0, shift=None, descale=None,
                         amax_out=None, heads_per_scale=1, colsum_part=None, dot_vec=None, heads_per_dot=1, dot_out=None, out=None):
    return _e4m3_meta(x, out)


def _register_op():
    global _op_lib
    if _op_lib is not None:
        return
    from . import flash_attn_interface  # noqa: F401  (defines the library this is a fragment of)
    lib = torch.library.Library("lite_attention", "FRAGMENT")
    lib.define(_QK_PREP_SCHEMA)
    lib.impl("qk_prep", _qk_prep_op, "CUDA")
    lib.impl("qk_prep", _qk_prep_meta, "Meta")
    lib.define(_QK_PREP_FP8_SCHEMA)
    lib.impl("qk_prep_fp8", _qk_prep_fp8_op, "CUDA")
    lib.impl("qk_prep_fp8", _qk_prep_fp8_meta, "Meta")
    lib.define(_QK_PREP_SMOOTH_SCHEMA)
    lib.impl("qk_prep_smooth", _qk_prep_smooth_op, "CUDA")
    lib.impl("qk_prep_smooth", _qk_prep_smooth_meta, "Meta")
    _op_lib = lib


_register_op()
