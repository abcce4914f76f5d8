"""V smoothing for the e4m3 forward. The kernel divides by its own row sum, so the rows of P sum to 1 over whatever keys a row visits -
with skip lists, with split keys and after an LSE merge - and ``P (V - 1 m^T) + 1 m^T = P V`` for any vector m per (batch, kv-head). V is
quantized as ``V - m``, the forward runs unchanged on the shifted codes, and m is added back to O in fp32:

    sv = SmoothedV()                                   # one per layer
    v8, dv, shift = sv(v_proj.view(b, s, n, d))        # e4m3 V - mean, its descale, the mean
    o, lse = flash_attn_func(q8, k8, v8, q_descale=dq, k_descale=dk, v_descale=dv, return_softmax_lse=True)
    o = sv.finish(o, lse=lse, out_dtype=torch.float32) # O + mean, as the fp32 the output projection reads

``v_colstats`` (``la_v_colstats`` + ``la_v_colstats_finish``) makes the mean and the exact amax of ``V - mean`` in ONE read of V;
``attn_unshift`` (``la_attn_unshift``) is the restoring pass, which also undoes K smoothing's shift of the LSE (``lse_unshift``, fused)
and casts. ``v_colstats_reference`` / ``attn_unshift_reference`` are the formulas in torch fp64; ``v_shift_as_bias`` folds the shift
into the bias of the output projection instead.

``v_prep_tiles`` (``la_v_prep_tiles``) is the quantizing pass for a V that only the attention call reads: it writes the e4m3 codes
straight into the V^T tiles the e4m3 forward stages and returns a ``PreparedV``, which ``flash_attn_func`` / ``LiteAttention`` take in
the place of ``v``; ``SmoothedV(tiles=True)`` and ``E4m3Scales(tiles=True)`` run it."""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import _cabi
from .qk_prep import _IN_DTYPES, _call, _check_scales, _check_x, _f32, descale_from_amax, qk_prep_smooth

_UNSHIFT_OUT_DTYPES = {torch.bfloat16: _cabi.LA_DTYPE_BF16, torch.float16: _cabi.LA_DTYPE_FP16, torch.float32: _cabi.LA_DTYPE_FP32}
_UNSHIFT_IN_DTYPES = {torch.bfloat16: _cabi.LA_DTYPE_BF16, torch.float16: _cabi.LA_DTYPE_FP16}


def v_colstats_parts(seqlen: int, num_heads: int, head_dim: int) -> Tuple[int, int]:
    """``(n_parts, rows_per_part)`` of ``v_colstats``'s partial statistics for a shape (``la_v_colstats_parts`` and
    ``la_v_colstats_part_rows``): part p holds rows ``[p * rows_per_part, (p + 1) * rows_per_part)`` of each batch. Pure functions of
    the shape: ``rows_per_part = max(16, ceil(S * H * D / 8 / 131072))``."""
    lib = _cabi.load()
    n = lib.la_v_colstats_parts(int(seqlen), int(num_heads), int(head_dim))
    r = lib.la_v_colstats_part_rows(int(seqlen), int(num_heads), int(head_dim))
    if n <= 0 or r <= 0:
        raise ValueError(f"la_v_colstats_parts({seqlen}, {num_heads}, {head_dim}): {_cabi.status_string(min(n, r))}")
    return n, r


def v_colstats(x: torch.Tensor, *, stat_part: Optional[torch.Tensor] = None, mean_out: Optional[torch.Tensor] = None,
               amax_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(mean, amax)`` of ``x`` (B, S, H, D) bf16 / fp16 / fp32 on the GPU in one read of it: ``mean`` fp32 (B, H, D) over the rows,
    ``amax`` fp32 (B, H) = the largest ``|fl(x - mean)|`` of the head - bit for bit what ``qk_prep_smooth(x, norm=None, shift=mean,
    amax_out=zeros, quantize=False)`` reports, without the second read. ``x`` may be any view whose last dimension is contiguous and
    whose rows, heads and batches start on 16-byte boundaries (the V slice of a fused projection); ``head_dim % 8 == 0``, at most 256.
    Deterministic (no float atomics). A NaN in a column makes that column's mean and the head's amax NaN.

    stat_part    fp32 (n_parts, 3, B, H, D) contiguous work buffer, ``n_parts`` from ``v_colstats_parts``; None: allocated.
    mean_out / amax_out   buffers to write (amax is WRITTEN, not accumulated); None: allocated.
    No host sync; with the three buffers given, no allocation; captures into a HIP graph."""
    _check_x(x, "v_colstats_reference")
    if x.stride(-1) != 1:
        raise ValueError("the last dimension of x must be contiguous")
    B, S, H, D = x.shape
    if B * S * H * D == 0:
        raise ValueError(f"x must not be empty, got {tuple(x.shape)}")
    n_parts, _ = v_colstats_parts(S, H, D)
    if stat_part is None:
        stat_part = torch.empty((n_parts, 3, B, H, D), dtype=torch.float32, device=x.device)
    _f32("stat_part", stat_part, (n_parts, 3, B, H, D), x.device)
    if not stat_part.is_contiguous():
        raise ValueError("stat_part must be contiguous")
    if mean_out is None:
        mean_out = torch.empty((B, H, D), dtype=torch.float32, device=x.device)
    _f32("mean_out", mean_out, (B, H, D), x.device)
    if mean_out.stride(2) != 1:
        raise ValueError("the last dimension of mean_out must be contiguous")
    if amax_out is None:
        amax_out = torch.empty((B, H), dtype=torch.float32, device=x.device)
    _f32("amax_out", amax_out, (B, H), x.device)
    a = _cabi.LaVColstatsArgs()
    a.struct_size = ctypes.sizeof(_cabi.LaVColstatsArgs)
    a.in_dtype = _IN_DTYPES[x.dtype]
    a.x, a.stat_part = x.data_ptr(), stat_part.data_ptr()
    a.x_batch_stride, a.x_row_stride, a.x_head_stride = x.stride(0), x.stride(1), x.stride(2)
    a.batch, a.seqlen, a.num_heads, a.head_dim = B, S, H, D
    _call("la_v_colstats", x, lambda: f"x {tuple(x.shape)} strides {x.stride()}", ctypes.byref(a))
    _call("la_v_colstats_finish", x, lambda: f"parts {tuple(stat_part.shape)}, seqlen {S}", stat_part.data_ptr(), n_parts, B, H, D, S,
          mean_out.data_ptr(), mean_out.stride(0), mean_out.stride(1), amax_out.data_ptr(), amax_out.stride(0), amax_out.stride(1))
    return mean_out, amax_out


def v_colstats_reference(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The formula of ``v_colstats`` in torch fp64, on whatever device ``x`` lives on: ``(mean`` (B, H, D) over the rows, ``amax`` (B, H)
    of ``|x - mean|)``."""
    if x.dim() != 4:
        raise ValueError(f"x must be (B, S, H, D), got {tuple(x.shape)}")
    y = x.double()
    mean = y.mean(dim=1)
    return mean, (y - mean[:, None]).abs().amax(dim=(1, 3))


def _check_unshift(o, shift, lse, lse_dot):
    """Shapes and dtypes of the restoring pass (device-free: LiteAttention checks with it before the forward). Returns heads_per_vec."""
    if o.dim() != 4:
        raise ValueError(f"o must be (B, S, H, D), got {tuple(o.shape)}")
    B, S, H, D = o.shape
    hpv = 1
    if shift is not None:
        if shift.dim() != 3 or shift.dtype != torch.float32 or shift.shape[0] != B or shift.shape[2] != D or shift.shape[1] < 1 or \
                H % shift.shape[1]:
            raise ValueError(f"shift must be fp32 (B, H_kv, D) = ({B}, a divisor of {H}, {D}), got {shift.dtype} {tuple(shift.shape)}")
        if shift.stride(2) != 1:
            raise ValueError("the last dimension of shift must be contiguous")
        hpv = H // shift.shape[1]
    for name, t in (("lse", lse), ("lse_dot", lse_dot)):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (B, H, S)):
            raise ValueError(f"{name} must be fp32 (B, H, S) = {(B, H, S)}, got {t.dtype} {tuple(t.shape)}")
    if lse_dot is not None and lse is None:
        raise ValueError("lse_dot needs lse")
    return hpv


def attn_unshift(o: torch.Tensor, shift: Optional[torch.Tensor] = None, *, lse: Optional[torch.Tensor] = None,
                 lse_dot: Optional[torch.Tensor] = None, softmax_scale: Optional[float] = None, out: Optional[torch.Tensor] = None,
                 out_dtype: Optional[torch.dtype] = None, lse_out: Optional[torch.Tensor] = None):
    """The restoring pass of V (and K) smoothing in one read of the attention output (``la_attn_unshift``):

        out[b, s, h]     = round(float(o[b, s, h]) + shift[b, h // (H_q // H_kv)])        one fp32 addition, one rounding
        lse_out[b, h, s] = lse[b, h, s] + softmax_scale * lse_dot[b, h, s]                 (one fma) only with ``lse_dot``

    o          bf16 / fp16 (B, S, H, D), what the attention call returned for the shifted V.
    shift      fp32 (B, H_kv, D), the vector subtracted from V; None: nothing is added (a cast / LSE pass).
    lse        fp32 (B, H, S) of the call. When given, a row whose lse is +-inf (the forward's empty sum: ``seqlen_k == 0`` gives O = 0,
               LSE = +inf) stays zeros and keeps its lse - no weights carry the shift. A NaN lse takes the normal path.
    lse_dot    fp32 (B, H, S), ``q . c`` of ``qk_prep_smooth`` / ``SmoothedQK``: ``lse_unshift`` fused. Needs ``lse``;
               ``softmax_scale`` is the one of the attention call (default ``head_dim ** -0.5``). ``lse_out``: where to (may be
               ``lse``); None: allocated.
    out        bf16, fp16 or fp32 by its own strides - e.g. a ``(B, S, H, D)`` view of the (B, S, H * D) fp32 tensor the output
               projection reads; may be ``o`` itself (in place); None: a new contiguous tensor of ``out_dtype`` (default ``o.dtype``).
               Any other overlap of ``out`` and ``o`` is an error nobody detects.
    Returns ``out``, or ``(out, lse_out)`` with ``lse_dot``. No host sync; no allocation when ``out`` (and ``lse_out``) are given;
    captures into a HIP graph."""
    hpv = _check_unshift(o, shift, lse, lse_dot)
    _check_x(o, "attn_unshift_reference", "o", _UNSHIFT_IN_DTYPES, "bf16 or fp16")
    B, S, H, D = o.shape
    if out is None:
        out = torch.empty((B, S, H, D), dtype=o.dtype if out_dtype is None else out_dtype, device=o.device)
    elif out_dtype is not None and out.dtype != out_dtype:
        raise TypeError(f"out is {out.dtype}, out_dtype says {out_dtype}")
    if out.dtype not in _UNSHIFT_OUT_DTYPES:
        raise TypeError(f"out: bf16, fp16 or fp32, got {out.dtype}")
    if out.shape != o.shape or out.device != o.device:
        raise ValueError(f"out must be {tuple(o.shape)} on {o.device}, got {tuple(out.shape)} on {out.device}")
    if o.stride(-1) != 1 or out.stride(-1) != 1:
        raise ValueError("the last dimension of o and out must be contiguous")
    for name, t in (("shift", shift), ("lse", lse), ("lse_dot", lse_dot), ("lse_out", lse_out)):
        if t is not None and t.device != o.device:
            raise ValueError(f"{name} lives on {t.device}, o on {o.device}")
    if lse_dot is not None:
        if lse_out is None:
            lse_out = torch.empty((B, H, S), dtype=torch.float32, device=o.device)
        _f32("lse_out", lse_out, (B, H, S), o.device)
    elif lse_out is not None:
        raise ValueError("lse_out needs lse_dot")
    for name, t in (("lse", lse), ("lse_dot", lse_dot), ("lse_out", lse_out)):
        if t is not None and not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    if B * S * H * D == 0:
        return out if lse_dot is None else (out, lse_out.copy_(lse))
    a = _cabi.LaAttnUnshiftArgs()
    a.struct_size = ctypes.sizeof(_cabi.LaAttnUnshiftArgs)
    a.o_dtype, a.out_dtype, a.heads_per_vec = _UNSHIFT_IN_DTYPES[o.dtype], _UNSHIFT_OUT_DTYPES[out.dtype], hpv
    a.o, a.out = o.data_ptr(), out.data_ptr()
    a.o_batch_stride, a.o_row_stride, a.o_head_stride = o.stride(0), o.stride(1), o.stride(2)
    a.out_batch_stride, a.out_row_stride, a.out_head_stride = out.stride(0), out.stride(1), out.stride(2)
    a.batch, a.seqlen, a.num_heads, a.head_dim = B, S, H, D
    if shift is not None:
        a.shift, a.shift_batch_stride, a.shift_head_stride = shift.data_ptr(), shift.stride(0), shift.stride(1)
    if lse is not None:
        a.lse = lse.data_ptr()
    if lse_dot is not None:
        a.lse_dot, a.lse_out = lse_dot.data_ptr(), lse_out.data_ptr()
        a.softmax_scale = float(D ** -0.5 if softmax_scale is None else softmax_scale)
    _call("la_attn_unshift", o, lambda: f"o {tuple(o.shape)} strides {o.stride()}, out {out.dtype} strides {out.stride()}, shift "
                                        f"{None if shift is None else (tuple(shift.shape), shift.stride())}", ctypes.byref(a))
    return out if lse_dot is None else (out, lse_out)


def attn_unshift_reference(o: torch.Tensor, shift: Optional[torch.Tensor] = None, *, lse: Optional[torch.Tensor] = None,
                           lse_dot: Optional[torch.Tensor] = None, softmax_scale: Optional[float] = None):
    """The formula of ``attn_unshift`` in torch fp64, UNROUNDED, on whatever device ``o`` lives on: ``out``, or ``(out, lse_out)`` with
    ``lse_dot``. The product ``softmax_scale * lse_dot`` takes the scale as the fp32 the kernel is handed."""
    hpv = _check_unshift(o, shift, lse, lse_dot)
    out = o.double()
    if shift is not None:
        out = out + shift.double().to(o.device).repeat_interleave(hpv, dim=1)[:, None]
    if lse is not None:
        out = torch.where(lse.to(o.device).isinf().transpose(1, 2)[..., None], torch.zeros_like(out), out)
    if lse_dot is None:
        return out
    scale = float(torch.tensor(o.shape[-1] ** -0.5 if softmax_scale is None else softmax_scale, dtype=torch.float32))
    l64 = lse.double()
    return out, torch.where(l64.isinf(), l64, l64 + scale * lse_dot.double())


# ---- O restored and row-scaled to e4m3 in one pass: la_attn_unshift_fp8 ----------------------------------------------------------------
ATTN_OUT_FP8_MAX_GROUP = 16384      # elements of a scale group (heads_per_scale * head_dim): a wave keeps them in registers
ATTN_OUT_FP8_MAX_HEADS = 1024


class RowScaledE4m3:
    """What ``attn_out_fp8`` returns: ``data`` float8_e4m3fn (B, S, H, D) and ``descale`` fp32 - (B, S, H / heads_per_scale) in the
    dynamic mode, the tensor that was given in the static one - with ``data.float() * descale`` (broadcast over a group) the restored
    O. ``data, descale = r`` unpacks."""

    __slots__ = ("data", "descale")

    def __init__(self, data: torch.Tensor, descale: torch.Tensor):
        self.data, self.descale = data, descale

    def __iter__(self):
        return iter((self.data, self.descale))

    def as_matrix(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(data.view(B * S, H * D), descale.view(B * S, 1))``: the activation and the row-wise scale a scaled GEMM over H * D takes.
        One scale per token (``heads_per_scale == H``) and contiguous tensors only; views, nothing is copied."""
        B, S, H, D = self.data.shape
        if tuple(self.descale.shape) != (B, S, 1):
            raise ValueError(f"as_matrix() needs one scale per token: descale (B, S, 1) = {(B, S, 1)}, got {tuple(self.descale.shape)}")
        if not self.data.is_contiguous() or not self.descale.is_contiguous():
            raise ValueError("as_matrix() needs contiguous data and descale")
        return self.data.view(B * S, H * D), self.descale.view(B * S, 1)


def _check_out_fp8(o, heads_per_scale, descale, amax_out):
    """Shapes and dtypes of the scale arguments of ``attn_out_fp8`` (device-free: the attention classes check with it before the
    forward). Returns heads_per_scale (None: H, one scale per token)."""
    B, S, H, D = o.shape
    hps = H if heads_per_scale is None else int(heads_per_scale)
    if hps < 1 or H % hps:
        raise ValueError(f"heads_per_scale must divide the {H} heads, got {heads_per_scale}")
    if hps * D > ATTN_OUT_FP8_MAX_GROUP:
        raise NotImplementedError(f"a scale group holds at most {ATTN_OUT_FP8_MAX_GROUP} elements, got heads_per_scale * head_dim = "
                                  f"{hps} * {D}")
    if H > ATTN_OUT_FP8_MAX_HEADS:
        raise NotImplementedError(f"at most {ATTN_OUT_FP8_MAX_HEADS} heads, got {H}")
    if D % 8:
        raise ValueError(f"head_dim must be a multiple of 8, got {D}")
    if descale is not None:
        if descale.dtype != torch.float32 or descale.numel() not in (1, B) or descale.dim() > 1:
            raise ValueError(f"descale must be fp32 of {B} elements (one per batch) or of one, got {descale.dtype} {tuple(descale.shape)}")
    if amax_out is not None:
        if descale is None:
            raise ValueError("amax_out is the running maximum of the static mode: it needs descale")
        if amax_out.dtype != torch.float32 or tuple(amax_out.shape) != (B,):
            raise ValueError(f"amax_out must be fp32 ({B},), got {amax_out.dtype} {tuple(amax_out.shape)}")
    return hps


def attn_out_fp8(o: torch.Tensor, shift: Optional[torch.Tensor] = None, *, lse: Optional[torch.Tensor] = None,
                 lse_dot: Optional[torch.Tensor] = None, softmax_scale: Optional[float] = None, heads_per_scale: Optional[int] = None,
                 descale: Optional[torch.Tensor] = None, amax_out: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                 descale_out: Optional[torch.Tensor] = None, lse_out: Optional[torch.Tensor] = None):
    """``attn_unshift`` with a row-scaled e4m3 result: the activation of an fp8 output projection in one read of O and one 1-byte
    write (``la_attn_unshift_fp8``). ``o``, ``shift``, ``lse``, ``lse_dot``, ``softmax_scale`` and ``lse_out`` are ``attn_unshift``'s;
    with y the fp32 value that pass would round:

        dynamic (``descale`` None)   descale[b, s, g] = max(max |y| over the group, 2^-100) / 448      g = h // heads_per_scale
        static  (``descale`` given)  fp32 of B elements or of one: a tensor-wise, delayed scale; ``amax_out`` fp32 (B,), ACCUMULATED as
                                     in ``qk_prep_fp8``, collects max |y| for the next step's scale (zero it for this call's)
        data = e4m3(clamp(y * (1 / descale), -448, 448))

    heads_per_scale   heads that share a scale; None: all H - ONE scale per token, what a row-wise scaled GEMM over H * D takes (not
                      one per head). ``heads_per_scale * head_dim <= 16384``.
    out               float8_e4m3fn (B, S, H, D) by its own strides, e.g. a view of a (B, S, H * D) buffer; never ``o`` (there is no
                      in-place form); None: allocated.
    descale_out       fp32 (B, S, H / heads_per_scale) by its own strides (dynamic mode); None: allocated.
    A NaN in a group makes that group's descale and bytes NaN and no other's. Returns ``RowScaledE4m3(data, descale)``, or
    ``(that, lse_out)`` with ``lse_dot``. No host sync; no allocation when the outputs are given; captures into a HIP graph."""
    hpv = _check_unshift(o, shift, lse, lse_dot)
    hps = _check_out_fp8(o, heads_per_scale, descale, amax_out)
    _check_x(o, "attn_out_fp8_reference", "o", _UNSHIFT_IN_DTYPES, "bf16 or fp16")
    B, S, H, D = o.shape
    G = H // hps
    if out is None:
        out = torch.empty((B, S, H, D), dtype=torch.float8_e4m3fn, device=o.device)
    if out.dtype != torch.float8_e4m3fn:
        raise TypeError(f"out: float8_e4m3fn, got {out.dtype}")
    if out.shape != o.shape or out.device != o.device:
        raise ValueError(f"out must be {tuple(o.shape)} on {o.device}, got {tuple(out.shape)} on {out.device}")
    if o.stride(-1) != 1 or out.stride(-1) != 1:
        raise ValueError("the last dimension of o and out must be contiguous")
    if descale is None:
        if descale_out is None:
            descale_out = torch.empty((B, S, G), dtype=torch.float32, device=o.device)
        _f32("descale_out", descale_out, (B, S, G), o.device)
    elif descale_out is not None:
        raise ValueError("descale_out is written in the dynamic mode only: descale was given")
    for name, t in (("shift", shift), ("lse", lse), ("lse_dot", lse_dot), ("lse_out", lse_out), ("descale", descale), ("amax_out", amax_out)):
        if t is not None and t.device != o.device:
            raise ValueError(f"{name} lives on {t.device}, o on {o.device}")
    if lse_dot is not None:
        if lse_out is None:
            lse_out = torch.empty((B, H, S), dtype=torch.float32, device=o.device)
        _f32("lse_out", lse_out, (B, H, S), o.device)
    elif lse_out is not None:
        raise ValueError("lse_out needs lse_dot")
    for name, t in (("lse", lse), ("lse_dot", lse_dot), ("lse_out", lse_out)):
        if t is not None and not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    res = RowScaledE4m3(out, descale_out if descale is None else descale)
    if B * S * H * D == 0:
        return res if lse_dot is None else (res, lse_out.copy_(lse))
    a = _cabi.LaAttnUnshiftFp8Args()
    a.struct_size = ctypes.sizeof(_cabi.LaAttnUnshiftFp8Args)
    a.o_dtype, a.heads_per_vec, a.heads_per_scale = _UNSHIFT_IN_DTYPES[o.dtype], hpv, hps
    a.o, a.out = o.data_ptr(), out.data_ptr()
    a.o_batch_stride, a.o_row_stride, a.o_head_stride = o.stride(0), o.stride(1), o.stride(2)
    a.out_batch_stride, a.out_row_stride, a.out_head_stride = out.stride(0), out.stride(1), out.stride(2)
    a.batch, a.seqlen, a.num_heads, a.head_dim = B, S, H, D
    if shift is not None:
        a.shift, a.shift_batch_stride, a.shift_head_stride = shift.data_ptr(), shift.stride(0), shift.stride(1)
    if lse is not None:
        a.lse = lse.data_ptr()
    if lse_dot is not None:
        a.lse_dot, a.lse_out = lse_dot.data_ptr(), lse_out.data_ptr()
        a.softmax_scale = float(D ** -0.5 if softmax_scale is None else softmax_scale)
    if descale is None:
        a.row_descale = descale_out.data_ptr()
        a.row_descale_batch_stride, a.row_descale_row_stride, a.row_descale_group_stride = descale_out.stride()
    else:
        a.descale_in = descale.data_ptr()
        a.descale_in_batch_stride = descale.stride(0) if descale.numel() > 1 else 0
        if amax_out is not None:
            a.amax, a.amax_batch_stride = amax_out.data_ptr(), amax_out.stride(0)
    _call("la_attn_unshift_fp8", o, lambda: f"o {tuple(o.shape)} strides {o.stride()}, out strides {out.stride()}, heads_per_scale {hps}, "
                                            f"shift {None if shift is None else (tuple(shift.shape), shift.stride())}", ctypes.byref(a))
    return res if lse_dot is None else (res, lse_out)


def attn_out_fp8_reference(o: torch.Tensor, shift: Optional[torch.Tensor] = None, *, lse: Optional[torch.Tensor] = None,
                           lse_dot: Optional[torch.Tensor] = None, softmax_scale: Optional[float] = None,
                           heads_per_scale: Optional[int] = None, descale: Optional[torch.Tensor] = None):
    """The formula of ``attn_out_fp8`` in torch fp64, UNROUNDED, on whatever device ``o`` lives on: ``(z, descale)`` with ``z = clamp(y /
    descale, -448, 448)`` fp64 (B, S, H, D) - the values the kernel rounds to e4m3 - and ``descale`` fp64 (B, S, H / heads_per_scale)
    = ``max(max |y|, 2^-100) / 448``, or the given one as fp64 (B, 1, 1); with ``lse_dot``, ``((z, descale), lse_out)``."""
    res = attn_unshift_reference(o, shift, lse=lse, lse_dot=lse_dot, softmax_scale=softmax_scale)
    y, lse_new = res if lse_dot is not None else (res, None)
    hps = _check_out_fp8(o, heads_per_scale, descale, None)
    B, S, H, D = y.shape
    if descale is None:
        d = y.reshape(B, S, H // hps, hps * D).abs().amax(dim=-1).clamp_min(2.0 ** -100) / 448.0
    else:
        d = descale.double().to(y.device).reshape(-1, 1, 1).expand(B, 1, 1)
    z = (y.reshape(B, S, -1, hps * D) / d[..., None]).clamp(-448.0, 448.0).reshape(B, S, H, D)
    return (z, d) if lse_dot is None else ((z, d), lse_new)


def v_shift_as_bias(weight: torch.Tensor, bias: Optional[torch.Tensor], shift: torch.Tensor,
                    dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """The zero-pass alternative to ``attn_unshift`` when nothing between the attention and its output projection needs the true O:
    the bias ``b' = b + W . flatten(shift repeated per q-head)`` under which ``F.linear(O_shifted.flatten(2), W, b')`` equals
    ``F.linear((O_shifted + shift).flatten(2), W, b)``.

    weight (out_features, H_q * D); bias (out_features,) or None; shift (1, H_kv, D) or (H_kv, D) - ONE batch's vector; H_q / H_kv is
    taken from the two shapes. Computed in ``promote_types(weight.dtype, float32)`` and returned so unless ``dtype`` is given. Pure
    torch, no host sync. It does NOT apply
      * to B > 1 with per-batch shifts (a bias is one vector; use ``attn_unshift``, or one bias per batch element by hand);
      * where partial outputs whose shifts differ are merged by LSE (sequence-parallel shards, the text + video recipe): each partial
        must be restored BEFORE the merge - the merge weights the shifts too;
      * to rows with an empty key set (their O is 0, not ``shift``), nor where anything between reads O."""
    if shift.dim() == 3:
        if shift.shape[0] != 1:
            raise ValueError(f"v_shift_as_bias folds ONE batch's shift into the bias, got shift {tuple(shift.shape)}: per-batch shifts need "
                             "attn_unshift")
        shift = shift[0]
    if shift.dim() != 2 or weight.dim() != 2:
        raise ValueError(f"weight (out_features, H_q * D) and shift (H_kv, D), got {tuple(weight.shape)} and {tuple(shift.shape)}")
    hkv, d = shift.shape
    if weight.shape[1] % (hkv * d):
        raise ValueError(f"the {weight.shape[1]} input features of weight are no multiple of H_kv * D = {hkv * d}")
    work = torch.promote_types(weight.dtype, torch.float32)
    vec = shift.to(device=weight.device, dtype=work).repeat_interleave(weight.shape[1] // (hkv * d), dim=0).reshape(-1)
    res = torch.mv(weight.to(work), vec)
    if bias is not None:
        res = res + bias.to(work)
    return res if dtype is None else res.to(dtype)


# ---- fp8 V in one pass: la_v_prep_tiles ------------------------------------------------------------------------------------------------
TILE_HEAD_DIMS = (64, 96, 128, 192, 256)      # the head dims the e4m3 forward has kernels for: the tile layouts there are


def v_tiles_bytes(batch: int, num_heads_k: int, seqlen_k: int, head_dim: int) -> Tuple[int, int]:
    """``(la_v_tiles_bytes, la_v_tiles_workspace_bytes)`` of a (B, Sk, Hk, D) V: the bytes of its V^T tiles, and of the workspace (the
    tiles, then the ticket counters) every fixed-length, unsplit e4m3 ``la_fwd`` over these keys accepts. Pure host functions."""
    lib = _cabi.load()
    args = (int(batch), int(num_heads_k), int(seqlen_k), int(head_dim))
    tiles, ws = lib.la_v_tiles_bytes(*args), lib.la_v_tiles_workspace_bytes(*args)
    if tiles < 0 or ws < 0:
        raise ValueError(f"la_v_tiles_bytes{args}: {_cabi.status_string(int(min(tiles, ws)))}")
    return int(tiles), int(ws)


class PreparedV:
    """A V that exists only as the V^T tiles of the e4m3 forward: what ``v_prep_tiles`` returns and ``flash_attn_func``,
    ``LiteAttention.__call__`` and ``LiteAttention.call_windowed`` accept as ``v`` / ``value``.

    workspace   1-D uint8, at least ``v_tiles_bytes(...)[1]`` bytes, 16-byte aligned: the tiles at its front, the forward's ticket
                counters behind them. The attention call launches ON this buffer (LA_FLAG_V_PREPARED, no allocation of its own); it
                belongs to whoever made it and must stay untouched until the attention calls that read it have run.
    shape       the logical ``(B, Sk, Hk, D)``; ``device`` is the workspace's.
    descale     the fp32 (B, Hk) descale it was quantized with (None: 1.0) - what the attention call wants as ``v_descale``."""

    __slots__ = ("workspace", "shape", "descale")

    def __init__(self, workspace: torch.Tensor, shape, descale: Optional[torch.Tensor] = None):
        shape = torch.Size(int(n) for n in shape)
        if len(shape) != 4 or min(shape) <= 0:
            raise ValueError(f"shape must be a non-empty (B, Sk, Hk, D), got {tuple(shape)}")
        if shape[3] not in TILE_HEAD_DIMS:
            raise NotImplementedError(f"V^T tiles exist for head_dim {TILE_HEAD_DIMS}, got {shape[3]} (a head_dim between them runs "
                                      "zero-padded: quantize into an e4m3 tensor instead)")
        need = v_tiles_bytes(shape[0], shape[2], shape[1], shape[3])[1]
        if workspace.dtype != torch.uint8 or workspace.dim() != 1 or not workspace.is_contiguous() or workspace.numel() < need:
            raise ValueError(f"workspace must be a contiguous 1-D uint8 tensor of at least {need} bytes, got {workspace.dtype} "
                             f"{tuple(workspace.shape)}")
        if workspace.data_ptr() % 16:
            raise ValueError("workspace must start on a 16-byte boundary")
        self.workspace, self.shape, self.descale = workspace, shape, descale

    @property
    def device(self) -> torch.device:
        return self.workspace.device

    def as_v(self) -> torch.Tensor:
        """An e4m3 (B, Sk, Hk, D) view of the front of the workspace: a buffer that passes the checks ``la_fwd`` makes of ``v`` (under
        LA_FLAG_V_PREPARED it is never read). Its bytes are tile bytes, NOT the codes in this order."""
        B, S, H, D = self.shape
        return self.workspace[: B * S * H * D].view(torch.float8_e4m3fn).view(B, S, H, D)

    def check_call(self, q, k, cu_seqlens_q=None, cu_seqlens_k=None, num_splits: int = 1):
        """Refuse, before anything is launched, the attention calls this V has no form for. Needs no device."""
        if cu_seqlens_q is not None or cu_seqlens_k is not None or q.dim() != 4 or k.dim() != 4:
            raise NotImplementedError("a PreparedV serves fixed-length (B, S, H, D) calls only: the tiles of a packed variable-length "
                                      "batch are laid out by its cu_seqlens")
        if q.dtype != torch.float8_e4m3fn or k.dtype != torch.float8_e4m3fn:
            raise ValueError(f"a PreparedV holds e4m3 tiles: q and k must be float8_e4m3fn, got {q.dtype} and {k.dtype}")
        if num_splits not in (0, 1):
            raise NotImplementedError("split-KV (num_splits > 1, or the host's choice -1) cuts the e4m3 V by rows, and a PreparedV has "
                                      "no such tensor")
        B, Sk, Hk, D = self.shape
        if tuple(k.shape) != (B, Sk, Hk, D) or q.shape[0] != B or q.shape[3] != D:
            raise ValueError(f"the PreparedV was made for k (B, Sk, Hk, D) = {(B, Sk, Hk, D)} and q (B, *, *, {D}), got k "
                             f"{tuple(k.shape)} and q {tuple(q.shape)}")
        if q.device != self.device or k.device != self.device:
            raise ValueError(f"the PreparedV lives on {self.device}, q on {q.device}, k on {k.device}")


def v_prep_tiles(x: torch.Tensor, *, descale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None,
                 amax_out: Optional[torch.Tensor] = None, out=None) -> PreparedV:
    """Quantize ``x`` (B, Sk, Hk, D) bf16 / fp16 / fp32 straight into the V^T tiles of the e4m3 forward (``la_v_prep_tiles``): one read
    of ``x``, one write of the tiles - the e4m3 (B, Sk, Hk, D) tensor of ``qk_prep_smooth(x, norm=None, ...)`` and the prepare pass the
    attention call runs over it drop out. Every code is the byte that pass would store:

        code = e4m3(clamp((float(x) - shift[b, h]) / descale[b, h], -448, 448))

    descale    fp32 (B, Hk); None: 1.0.       shift   fp32 (B, Hk, D), last dimension contiguous; None: none.
    amax_out   fp32 (B, Hk), ACCUMULATED as in ``qk_prep_fp8``: the running maximum of ``|x - shift|`` (zero it for this call's).
    out        a ``PreparedV`` of this shape, or its 1-D uint8 workspace (at least ``v_tiles_bytes(B, Hk, Sk, D)[1]`` bytes, 16-byte
               aligned), to write into; None: allocated.
    ``x`` may be any view whose last dimension is contiguous and whose rows, heads and batches start on 16-byte boundaries (the V
    slice of a fused projection); head_dim 64, 96, 128, 192 or 256. No host sync; with ``out`` given, no allocation; captures into
    a HIP graph; two calls write the same bytes."""
    _check_x(x, "v_prep_tiles_reference")
    if x.stride(-1) != 1:
        raise ValueError("the last dimension of x must be contiguous")
    B, S, H, D = x.shape
    if B * S * H * D == 0:
        raise ValueError(f"x must not be empty, got {tuple(x.shape)}")
    _check_scales(x, 1, descale, amax_out)
    if shift is not None:
        _f32("shift", shift, (B, H, D), x.device)
        if shift.stride(2) != 1:
            raise ValueError("the last dimension of shift must be contiguous")
    if isinstance(out, PreparedV):
        if out.shape != x.shape or out.device != x.device:
            raise ValueError(f"out was made for {tuple(out.shape)} on {out.device}, x is {tuple(x.shape)} on {x.device}")
        out.descale = descale
        pv = out
    else:
        if out is None:
            out = torch.empty(v_tiles_bytes(B, H, S, D)[1], dtype=torch.uint8, device=x.device)
        elif out.device != x.device:
            raise ValueError(f"out lives on {out.device}, x on {x.device}")
        pv = PreparedV(out, x.shape, descale)
    a = _cabi.LaVPrepTilesArgs()
    a.struct_size = ctypes.sizeof(_cabi.LaVPrepTilesArgs)
    a.in_dtype = _IN_DTYPES[x.dtype]
    a.x, a.tiles = x.data_ptr(), pv.workspace.data_ptr()
    a.x_batch_stride, a.x_row_stride, a.x_head_stride = x.stride(0), x.stride(1), x.stride(2)
    a.batch, a.seqlen, a.num_heads, a.head_dim = B, S, H, D
    if descale is not None:
        a.descale, a.descale_batch_stride, a.descale_head_stride = descale.data_ptr(), descale.stride(0), descale.stride(1)
    if shift is not None:
        a.shift, a.shift_batch_stride, a.shift_head_stride = shift.data_ptr(), shift.stride(0), shift.stride(1)
    if amax_out is not None:
        a.amax, a.amax_batch_stride, a.amax_head_stride = amax_out.data_ptr(), amax_out.stride(0), amax_out.stride(1)
    _call("la_v_prep_tiles", x, lambda: f"x {tuple(x.shape)} strides {x.stride()}, shift "
                                        f"{None if shift is None else shift.stride()}", ctypes.byref(a))
    return pv


def v_prep_tiles_reference(x: torch.Tensor, *, descale: Optional[torch.Tensor] = None,
                           shift: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The e4m3 codes ``v_prep_tiles`` puts into the tiles, in (B, Sk, Hk, D) order, by the same fp32 steps in torch on whatever device
    ``x`` lives on: one subtraction, one multiplication by the fp32 ``1 / descale``, the clamp, torch's round-to-nearest-even cast."""
    if x.dim() != 4:
        raise ValueError(f"x must be (B, S, H, D), got {tuple(x.shape)}")
    y = x.float()
    if shift is not None:
        y = y - shift.to(y.device)[:, None]
    if descale is not None:
        y = y * (1.0 / descale.to(y.device))[:, None, :, None]
    return y.clamp(-448.0, 448.0).to(torch.float8_e4m3fn)


class SmoothedV:
    """The buffers of one layer's V across calls, mean-shifted before it is quantized: ``v8, dv, shift = sv(xv)`` - ``v8`` e4m3 of
    ``xv - shift``, ``dv`` its descale for the attention call, ``shift`` fp32 (B, H_kv, D) - and ``sv.finish(o, ...)`` adds the shift
    back to what the attention call returned (``attn_unshift``).

    mode "current"   ``v_colstats`` (mean and exact amax of ``xv - mean``), ``descale_from_amax``, the quantizing pass
                     (``qk_prep_smooth`` with ``norm=None``): two reads of xv.
    mode "delayed"   step t quantizes with step t - 1's mean and descale and runs ``v_colstats`` on the same input for step t + 1. ANY
                     shift is exact, so a stale mean costs range only (what outgrows ``margin`` saturates at +-448), as ``SmoothedQK``
                     documents. The first call has no history and runs as "current".
    tiles=True       the quantizing pass is ``v_prep_tiles``: ``v8`` is a ``PreparedV`` (the V^T tiles of the e4m3 forward, no e4m3
                     tensor), which the attention call takes as ``v``. Head_dim 64, 96, 128, 192 or 256.
    Buffers are allocated by the first call and reused: no host sync, no allocation after it; a call overwrites the last results,
    ``shift`` included - call ``finish`` before the next ``sv(xv)``."""

    def __init__(self, mode: str = "current", margin: float = 1.0, tiles: bool = False):
        if mode not in ("current", "delayed"):
            raise ValueError('mode: "current" or "delayed"')
        if not margin > 0:
            raise ValueError("margin must be positive")
        self.mode, self.margin, self.tiles = mode, float(margin), bool(tiles)
        self.v8 = self.shift = self.out = self.out8 = self.out_descale = None
        self.calls = 0

    def _allocate(self, xv):
        B, S, H, D = xv.shape
        f32 = dict(dtype=torch.float32, device=xv.device)
        if self.tiles:
            self.v8 = PreparedV(torch.empty(v_tiles_bytes(B, H, S, D)[1], dtype=torch.uint8, device=xv.device), xv.shape)
        else:
            self.v8 = torch.empty(xv.shape, dtype=torch.float8_e4m3fn, device=xv.device)
        self.part = torch.empty((v_colstats_parts(S, H, D)[0], 3, B, H, D), **f32)
        self.shift, self.amax, self.dv = torch.empty((B, H, D), **f32), torch.empty((B, H), **f32), torch.empty((B, H), **f32)
        if self.mode == "delayed":                               # this step's statistics, for the next step
            self.next_mean, self.next_amax = torch.empty_like(self.shift), torch.empty_like(self.amax)
        self.out = None

    def __call__(self, xv: torch.Tensor):
        if xv.dim() != 4:
            raise ValueError(f"xv must be (B, S, H, D), got {tuple(xv.shape)}")
        first = self.v8 is None or self.v8.shape != xv.shape or self.v8.device != xv.device
        if first:
            self._allocate(xv)
        if self.mode == "current":
            v_colstats(xv, stat_part=self.part, mean_out=self.shift, amax_out=self.amax)
        else:
            if first:
                v_colstats(xv, stat_part=self.part, mean_out=self.next_mean, amax_out=self.next_amax)
            self.shift.copy_(self.next_mean)
            self.amax.copy_(self.next_amax)
        descale_from_amax(self.amax, self.margin, out=self.dv)
        if self.tiles:
            v_prep_tiles(xv, shift=self.shift, descale=self.dv, out=self.v8)
        else:
            qk_prep_smooth(xv, norm=None, shift=self.shift, descale=self.dv, out=self.v8)
        if self.mode == "delayed":
            v_colstats(xv, stat_part=self.part, mean_out=self.next_mean, amax_out=self.next_amax)
        self.calls += 1
        return self.v8, self.dv, self.shift

    def finish(self, o: torch.Tensor, lse: Optional[torch.Tensor] = None, lse_dot: Optional[torch.Tensor] = None,
               softmax_scale: Optional[float] = None, out: Optional[torch.Tensor] = None, out_dtype: Optional[torch.dtype] = None,
               *, fp8: bool = False, heads_per_scale: Optional[int] = None, descale: Optional[torch.Tensor] = None):
        """``attn_unshift(o, shift, ...)`` with the shift of the last call. ``out`` None: ``o`` itself when ``out_dtype`` is None or
        ``o.dtype`` (in place: the attention call's result is overwritten), else a buffer of ``out_dtype`` this object keeps. With
        ``lse_dot`` (K smoothed too) the LSE is restored in place and ``(out, lse)`` is returned. Pass ``lse`` whenever the call may
        have had no keys.
        ``fp8=True``: ``attn_out_fp8(o, shift, ..., heads_per_scale=, descale=)`` instead - a ``RowScaledE4m3`` whose buffers this
        object keeps (``out``: the e4m3 tensor to write; ``out_dtype`` must be None)."""
        if self.shift is None:
            raise RuntimeError("finish() before the first call: there is no shift yet")
        if fp8:
            if out_dtype is not None:
                raise ValueError("fp8=True writes e4m3: out_dtype must be None")
            _check_unshift(o, self.shift, lse, lse_dot)
            hps = _check_out_fp8(o, heads_per_scale, descale, None)
            if out is None:
                if self.out8 is None or self.out8.shape != o.shape or self.out8.device != o.device:
                    self.out8 = torch.empty(o.shape, dtype=torch.float8_e4m3fn, device=o.device)
                out = self.out8
            want = (o.shape[0], o.shape[1], o.shape[2] // hps)
            if descale is None and (self.out_descale is None or tuple(self.out_descale.shape) != want or self.out_descale.device != o.device):
                self.out_descale = torch.empty(want, dtype=torch.float32, device=o.device)
            return attn_out_fp8(o, self.shift, lse=lse, lse_dot=lse_dot, softmax_scale=softmax_scale, heads_per_scale=hps, descale=descale,
                                out=out, descale_out=self.out_descale if descale is None else None,
                                lse_out=lse if lse_dot is not None else None)
        if heads_per_scale is not None or descale is not None:
            raise ValueError("heads_per_scale and descale belong to fp8=True")
        if out is None:
            if out_dtype is None or out_dtype == o.dtype:
                out = o
            else:
                if self.out is None or self.out.shape != o.shape or self.out.dtype != out_dtype or self.out.device != o.device:
                    self.out = torch.empty(o.shape, dtype=out_dtype, device=o.device)
                out = self.out
        return attn_unshift(o, self.shift, lse=lse, lse_dot=lse_dot, softmax_scale=softmax_scale, out=out, out_dtype=out_dtype,
                            lse_out=lse if lse_dot is not None else None)


# ---- op registration: torch.ops.lite_attention.v_colstats / attn_unshift / v_prep_tiles, beside qk_prep_smooth ------------------------------------------
_V_COLSTATS_SCHEMA = ("v_colstats(Tensor x, Tensor(part!)? stat_part = None, Tensor(mean!)? mean_out = None, "
                      "Tensor(amax!)? amax_out = None) -> (Tensor(mean!), Tensor(amax!))")
_ATTN_UNSHIFT_SCHEMA = ("attn_unshift(Tensor o, Tensor? shift = None, Tensor? lse = None, Tensor? lse_dot = None, "
                        "float? softmax_scale = None, Tensor(out!)? out = None, ScalarType? out_dtype = None, "
                        "Tensor(lse_out!)? lse_out = None) -> Tensor(out!)")
_V_PREP_TILES_SCHEMA = ("v_prep_tiles(Tensor x, Tensor? descale = None, Tensor? shift = None, Tensor(amax!)? amax_out = None, "
                        "Tensor(out!)? out = None) -> Tensor(out!)")
_op_lib = None


def _v_prep_tiles_op(x, descale=None, shift=None, amax_out=None, out=None):
    """The op speaks tensors: ``out`` and the result are the uint8 workspace (``PreparedV(result, x.shape, descale)`` wraps it)."""
    return v_prep_tiles(x, descale=descale, shift=shift, amax_out=amax_out, out=out).workspace


def _v_prep_tiles_meta(x, descale=None, shift=None, amax_out=None, out=None):
    """Shape and dtype only."""
    B, S, H, D = x.shape
    return out if out is not None else torch.empty(v_tiles_bytes(B, H, S, D)[1], dtype=torch.uint8, device=x.device)


def _v_colstats_op(x, stat_part=None, mean_out=None, amax_out=None):
    return v_colstats(x, stat_part=stat_part, mean_out=mean_out, amax_out=amax_out)


def _v_colstats_meta(x, stat_part=None, mean_out=None, amax_out=None):
    """Shapes and dtypes only (fake-tensor tracing treats the op as opaque)."""
    B, _, H, D = x.shape
    return (mean_out if mean_out is not None else torch.empty((B, H, D), dtype=torch.float32, device=x.device),
            amax_out if amax_out is not None else torch.empty((B, H), dtype=torch.float32, device=x.device))


def _attn_unshift_op(o, shift=None, lse=None, lse_dot=None, softmax_scale=None, out=None, out_dtype=None, lse_out=None):
    """The op returns ``out``; with ``lse_dot`` it wants ``lse_out`` too and writes the LSE there."""
    if lse_dot is not None and lse_out is None:
        raise ValueError("the op writes the LSE into lse_out: give it")
    res = attn_unshift(o, shift, lse=lse, lse_dot=lse_dot, softmax_scale=softmax_scale, out=out, out_dtype=out_dtype, lse_out=lse_out)
    return res if lse_dot is None else res[0]


def _attn_unshift_meta(o, shift=None, lse=None, lse_dot=None, softmax_scale=None, out=None, out_dtype=None, lse_out=None):
    """Shape and dtype only."""
    return out if out is not None else torch.empty(o.shape, dtype=o.dtype if out_dtype is None else out_dtype, device=o.device)


_ATTN_OUT_FP8_SCHEMA = ("attn_out_fp8(Tensor o, Tensor? shift = None, Tensor? lse = None, Tensor? lse_dot = None, "
                        "float? softmax_scale = None, int? heads_per_scale = None, Tensor? descale = None, "
                        "Tensor(amax!)? amax_out = None, Tensor(out!)? out = None, Tensor(ds!)? descale_out = None, "
                        "Tensor(lse_out!)? lse_out = None) -> (Tensor, Tensor)")


def _attn_out_fp8_op(o, shift=None, lse=None, lse_dot=None, softmax_scale=None, heads_per_scale=None, descale=None, amax_out=None,
                     out=None, descale_out=None, lse_out=None):
    """The op returns ``(data, descale)``; with ``lse_dot`` it wants ``lse_out`` too and writes the LSE there. What it returns are new
    tensors on the given storage (an op may not return its arguments)."""
    if lse_dot is not None and lse_out is None:
        raise ValueError("the op writes the LSE into lse_out: give it")
    res = attn_out_fp8(o, shift, lse=lse, lse_dot=lse_dot, softmax_scale=softmax_scale, heads_per_scale=heads_per_scale, descale=descale,
                       amax_out=amax_out, out=out, descale_out=descale_out, lse_out=lse_out)
    res = res if lse_dot is None else res[0]
    return res.data.view(res.data.shape), res.descale.view(res.descale.shape)


def _attn_out_fp8_meta(o, shift=None, lse=None, lse_dot=None, softmax_scale=None, heads_per_scale=None, descale=None, amax_out=None,
                       out=None, descale_out=None, lse_out=None):
    """Shapes and dtypes only."""
    B, S, H, _ = o.shape
    hps = H if heads_per_scale is None else heads_per_scale
    return (torch.empty(o.shape, dtype=torch.float8_e4m3fn, device=o.device),
            torch.empty((B, S, H // hps) if descale is None else descale.shape, dtype=torch.float32, device=o.device))


def _register_op():
    global _op_lib
    if _op_lib is not None:
        return
    from . import flash_attn_interface  # noqa: F401  (defines the library this is a fragment of)
    lib = torch.library.Library("lite_attention", "FRAGMENT")
    lib.define(_V_COLSTATS_SCHEMA)
    lib.impl("v_colstats", _v_colstats_op, "CUDA")
    lib.impl("v_colstats", _v_colstats_meta, "Meta")
    lib.define(_ATTN_UNSHIFT_SCHEMA)
    lib.impl("attn_unshift", _attn_unshift_op, "CUDA")
    lib.impl("attn_unshift", _attn_unshift_meta, "Meta")
    lib.define(_ATTN_OUT_FP8_SCHEMA)
    lib.impl("attn_out_fp8", _attn_out_fp8_op, "CUDA")
    lib.impl("attn_out_fp8", _attn_out_fp8_meta, "Meta")
    lib.define(_V_PREP_TILES_SCHEMA)
    lib.impl("v_prep_tiles", _v_prep_tiles_op, "CUDA")
    lib.impl("v_prep_tiles", _v_prep_tiles_meta, "Meta")
    _op_lib = lib


_register_op()
