"""The arithmetic of la_attn_unshift_fp8 step by step in torch fp32 on the CPU - the expected bytes and descales of
tests/test_gpu_attn_out_fp8.py, checked against the fp64 reference by tests/test_attn_out_fp8_cpu.py. Every step is one correctly
rounded fp32 operation, as in the kernel: the addition of the shift, the maximum of |y| (order free), clamp_min(2^-100) / 448, the
reciprocal, the product, the clamp, torch's round-to-nearest-even cast to e4m3. Nothing here calls the code under test."""
import torch

F8 = torch.float8_e4m3fn
TINY = 2.0 ** -100


def restored(o, shift=None, lse=None):
    """y of attn_unshift in fp32, unrounded: float(o) + shift of the row's kv head, zeros where the head's lse is +-inf."""
    y = o.detach().cpu().float()
    H = y.shape[2]
    if shift is not None:
        s = shift.detach().cpu()
        y = y + s.repeat_interleave(H // s.shape[1], dim=1)[:, None]
    if lse is not None:
        y = torch.where(lse.detach().cpu().isinf().transpose(1, 2)[..., None], torch.zeros_like(y), y)
    return y


def emulate(o, shift=None, lse=None, heads_per_scale=None, descale=None):
    """(data e4m3 (B, S, H, D), descale fp32 (B, S, H / hps) - or the given one -, y fp32) on the CPU."""
    y = restored(o, shift, lse)
    B, S, H, D = y.shape
    hps = H if heads_per_scale is None else heads_per_scale
    yg = y.reshape(B, S, H // hps, hps * D)
    if descale is None:
        d = yg.abs().amax(dim=-1).clamp_min(TINY) / 448.0              # a NaN in the group: NaN
        inv = (1.0 / d)[..., None]
    else:
        d = descale.detach().cpu()
        inv = (1.0 / d.reshape(-1, 1, 1).expand(B, 1, 1))[..., None]
    assert inv.dtype == torch.float32
    data = (yg * inv).clamp(-448.0, 448.0).to(F8).reshape(B, S, H, D)
    return data, d, y
