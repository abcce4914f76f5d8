"""A CPU emulation of the e4m3 forward, for the error bounds of V smoothing: per-head e4m3 q / k / v (torch's ``float8_e4m3fn`` cast,
current scaling), scores and exp in fp64, P in fp32 or rounded to e4m3, row sums of the unrounded or of the rounded P. The forward
stores its O in bf16, as the device does; ``out_dtype`` is the type the restoring pass (or, without smoothing, a plain cast) hands on.
It models the rounding of the operands, of P and of O - not the device's own exp or its accumulation order.

``smoothing_ratio`` is what the tests assert on: the relative rms error of O against fp64 with V mean-shifted, over the error without,
on the case of tests/test_gpu_qk_prep_smooth.py with the offset on V."""
import torch

F8 = torch.float8_e4m3fn
E4M3_MAX = 448.0


def quantize_per_head(x):
    """(codes as fp64, descale (B, H)) of x (B, S, H, D): amax / 448 per (batch, head), round to nearest even e4m3."""
    d = x.abs().amax(dim=(1, 3)).clamp_min(2.0 ** -100).float() / E4M3_MAX
    codes = (x.float() / d[:, None, :, None]).clamp(-E4M3_MAX, E4M3_MAX).to(F8).double()
    return codes, d.double()


def fp8_attention_emulation(q, k, v, *, smooth_v=False, round_p=True, rowsum_of_rounded_p=False, out_dtype=torch.bfloat16, scale=None):
    """O (B, S, H, D) in ``out_dtype`` of the emulated e4m3 attention of q, k, v (B, S, H, D; their values are taken as given).
    smooth_v: V is quantized as ``fl32(V - mean32)``, the fp32 mean over the rows, and the mean is added in fp32 to the bf16 O of the
    forward, then rounded to ``out_dtype``. round_p: ``exp(s - max)`` (at most 1) is rounded to e4m3 before the PV product.
    rowsum_of_rounded_p: the row sum is taken of the rounded P (the matrix-pipe form) instead of the unrounded one (the default form
    of the kernels)."""
    D = q.shape[-1]
    scale = D ** -0.5 if scale is None else scale
    q8, dq = quantize_per_head(q)
    k8, dk = quantize_per_head(k)
    vf = v.float()
    mean = vf.mean(dim=1) if smooth_v else None
    v8, dv = quantize_per_head(vf - mean[:, None] if smooth_v else vf)
    s = torch.einsum("bqhd,bkhd->bhqk", q8, k8) * (dq * dk)[:, :, None, None] * scale
    p = torch.exp(s - s.amax(dim=-1, keepdim=True))
    p_used = p.float().to(F8).double() if round_p else p.float().double()
    l = (p_used if (round_p and rowsum_of_rounded_p) else p.float().double()).sum(dim=-1)
    o = torch.einsum("bhqk,bkhd->bqhd", p_used, v8) * dv[:, None, :, None] / l.transpose(1, 2)[..., None]
    o = o.float().bfloat16().float()                           # what the forward stores
    if smooth_v:
        o = o + mean[:, None]                                  # the restoring pass: one fp32 addition, one rounding
    return o.to(out_dtype)


def offset_vector(H, D, size, seed):
    """+-size on 8 channels of every head, sign and channel drawn per head (tests/test_gpu_qk_prep_smooth.py's)."""
    g = torch.Generator().manual_seed(seed)
    c = torch.zeros(H, D)
    for h in range(H):
        idx = torch.randperm(D, generator=g)[:8]
        c[h, idx] = size * (2.0 * torch.randint(0, 2, (8,), generator=g) - 1.0)
    return c


_CASES = {}


def case(offset):
    """B = 1, S = 320, H = 2, D = 128, bf16 q / k / v on the CPU, +-offset on 8 channels of every V head, and the fp64 attention output
    of those bf16 values; computed once."""
    if offset not in _CASES:
        g = torch.Generator().manual_seed(0)
        q, k, v = (torch.randn(1, 320, 2, 128, generator=g) for _ in range(3))
        v = v + offset_vector(2, 128, float(offset), 1)[None, None]
        q, k, v = (t.bfloat16() for t in (q, k, v))
        s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) * 128 ** -0.5
        o64 = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, dim=-1), v.double())
        _CASES[offset] = (q, k, v, o64, torch.logsumexp(s, dim=-1))
    return _CASES[offset]


def rel_rms(got, ref):
    return ((got.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


_RATIOS = {}


def smoothing_ratio(offset, out_dtype=torch.bfloat16, round_p=True, rowsum_of_rounded_p=False):
    """(error with smoothing / error without, the two errors) of the emulation on ``case(offset)``."""
    key = (offset, out_dtype, round_p, rowsum_of_rounded_p)
    if key not in _RATIOS:
        q, k, v, o64, _ = case(offset)
        kw = dict(round_p=round_p, rowsum_of_rounded_p=rowsum_of_rounded_p, out_dtype=out_dtype)
        plain = rel_rms(fp8_attention_emulation(q, k, v, smooth_v=False, **kw), o64)
        smooth = rel_rms(fp8_attention_emulation(q, k, v, smooth_v=True, **kw), o64)
        _RATIOS[key] = (smooth / plain, plain, smooth)
    return _RATIOS[key]
