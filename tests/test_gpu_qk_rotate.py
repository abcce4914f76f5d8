"""GPU: head rotation in the q / k prologue (`rotate=`, la_qk_prep_rot and its e4m3 and smoothing forms) against the fp64 references
(every head times the dense M). The rotation's own error term, per element: E = 2^-19 |y_head|_2 - at most 8 butterfly stages and the
scale, each one fp32 rounding of an intermediate bounded, after the 1 / sqrt(D), by |y_head|_2 (under 2^-20 |y_head|_2 together),
doubled for the few fp32 ulps y carries from norm and rope. 16-bit out: half an ulp of the out dtype at y64 + E. The e4m3 and smoothing
forms: the rules of tests/test_gpu_qk_prep_smooth.py with E where an unrotated element has its fp32 term 2^-16 pair_sum. The LSE:
0.084 on the input that file holds the bound to, N(0, 1) rows of 320 keys (on 9-key rows with per-head scales up to 4 the operands'
own e4m3 rounding moves single scores by more, rotated or not: 0.106 rotated, 0.122 unrotated smoothed, 0.184 unrotated plain)."""
import pytest
import torch

import test_gpu_qk_prep_smooth as smooth

pytestmark = pytest.mark.gpu
GRID = (1, 3, 3)
B, S = 2, 9                                                      # a last round of four tokens with three spare waves
# form -> norm; H = 5: one wave per token, and the head kernel with 64 / G heads per pass not dividing H; token_wg: H D > 5120, a workgroup per token
NORMS = {"token": "token", "token_wg": "token", "head": "head", "none": None}
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def setup(D, form, dtype=BF, seed=0, H=None):
    import liteattention_amd as L
    H = (5120 // D + 8 if form == "token_wg" else 5) if H is None else H
    x, w = smooth.make_x(B, S, H, D, dtype, seed=seed + D)
    return x, smooth.weight_for(w, NORMS[form], D), L.rope_tables(GRID, D, device="cuda"), NORMS[form], L.head_rotation(D, seed=D, device="cuda")


def rot_err(y64):
    return 2.0 ** -19 * y64.norm(dim=-1, keepdim=True)


def half_ulp(y64, dtype):
    mant, least = (8, -134) if dtype == torch.bfloat16 else (11, -25)
    return torch.exp2((torch.frexp(y64)[1] - 1 - mant).clamp_min(least).double())


@pytest.mark.parametrize("D,form,in_dtype,out_dtype,extra", [(D, f, i, o, "") for D in (64, 128, 256) for f in NORMS for i, o in ((BF, BF), (F32, F16))]
                         + [(64, "token", BF, BF, "rows"), (128, "head", BF, BF, "rows"), (128, "token_wg", BF, BF, "in_place"),
                            (256, "head", BF, BF, "in_place"), (256, "token", BF, BF, "no_signs")])
def test_the_rotation_against_fp64(D, form, in_dtype, out_dtype, extra):
    import liteattention_amd as L
    x, w, tables, norm, rot = setup(D, form, in_dtype)
    kw = {}
    if extra == "no_signs":
        rot = L.head_rotation(D, signs=False, device="cuda")
    if extra == "rows":
        kw = dict(rows=torch.tensor([8, 0, 3, 3, 7], dtype=torch.int32).cuda(), positions=torch.tensor([1, 8, 0, 5, 2], dtype=torch.int32).cuda())
    ref = L.qk_prep_reference(x, w, 1e-6, tables, norm, rotate=rot, **kw)
    plain = L.qk_prep(x, w, 1e-6, tables, norm, out_dtype=out_dtype, **kw)
    assert torch.equal(L.qk_prep(x, w, 1e-6, tables, norm, out_dtype=out_dtype, rotate=None, **kw), plain)
    out = L.qk_prep(x, w, 1e-6, tables, norm, out_dtype=out_dtype, rotate=rot, **kw)
    assert torch.equal(L.qk_prep(x, w, 1e-6, tables, norm, out_dtype=out_dtype, rotate=rot, **kw), out)      # two launches: the same bits
    if extra == "in_place":
        buf = x.clone()
        assert L.qk_prep(buf, w, 1e-6, tables, norm, out=buf, rotate=rot) is buf and torch.equal(buf, out)
    ratio = ((out.double() - ref).abs() / (half_ulp(ref, out_dtype) + rot_err(ref))).max().item()
    print(f"D {D} {form} {in_dtype} -> {out_dtype} {extra}: max err / bound {ratio:.3f}")
    assert ratio <= 1.0 and (out.double() - plain.double()).abs().max().item() > 0.1


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("form", ["token", "head"])
def test_the_e4m3_and_smoothing_forms_and_the_lse(D, form):
    """GQA: 4 query heads on 2 key heads, heads_per_scale = heads_per_dot = 2 for q."""
    import liteattention_amd as L
    xq, wq, tables, norm, rot = setup(D, form, H=4)
    xk, wk = setup(D, form, seed=1, H=2)[:2]
    args_q, args_k = (xq, wq, 1e-6, tables, norm), (xk, wk, 1e-6, tables, norm)
    # k: the mean of the rotated keys, then shifted codes and amax; q: amax, codes and the dots with that mean
    n_parts, rows = L.qk_prep_smooth_parts(S, 2, D)
    _, _, mean64, _ = L.qk_prep_smooth_reference(*args_k, rotate=rot)
    mean = L.qk_prep_colmean(*args_k, rotate=rot)
    yk, yq = L.qk_prep_reference(*args_k, rotate=rot), L.qk_prep_reference(*args_q, rotate=rot)
    assert ((mean.double() - mean64).abs() <= rot_err(yk).expand_as(yk).mean(1) + (rows + n_parts) * 2.0 ** -24 * yk.abs().mean(1) + 1e-7).all()
    for x_args, y, hps, shift, dot_vec in ((args_k, yk, 1, mean, None), (args_q, yq, 2, None, mean)):
        z1, amax64, _, dots64 = L.qk_prep_smooth_reference(*x_args, shift=shift, heads_per_scale=hps, dot_vec=dot_vec, heads_per_dot=2, rotate=rot)
        H, sh = y.shape[2], torch.zeros_like(y[:, 0]) if shift is None else shift.double()
        descale = (amax64.clamp_min(1e-3) / 448.0 * 1.5).float()
        d_el = descale.double().repeat_interleave(hps, dim=1)[:, None, :, None]
        amax = torch.zeros(B, H // hps, device="cuda")
        dot_out = None if dot_vec is None else torch.empty(B, H, S, device="cuda")
        out = L.qk_prep_smooth(*x_args, shift=shift, descale=descale, amax_out=amax, heads_per_scale=hps, dot_vec=dot_vec, heads_per_dot=2,
                               dot_out=dot_out, rotate=rot)
        E, z = rot_err(y).expand_as(y), (z1 / d_el).clamp(-448, 448)
        assert ((out.double() - z).abs() <= 2.0 ** -4 * z.abs() + 2.0 ** -10 + E / d_el + 2.0 ** -24 * sh.abs()[:, None] / d_el + 1e-7).all()
        a_bound = E.reshape(B, S, H // hps, -1).amax(dim=(1, 3)) + 2.0 ** -24 * sh.abs().reshape(B, H // hps, -1).amax(2) + 1e-7
        assert ((amax.double() - amax64).abs() <= a_bound).all()
        if shift is None:                                        # without a shift the e4m3 form computes the same amax and the same codes
            assert torch.equal(L.qk_prep_amax(*x_args, heads_per_scale=hps, rotate=rot), amax)
            assert torch.equal(L.qk_prep_fp8(*x_args, descale=descale, heads_per_scale=hps, rotate=rot).view(torch.uint8), out.view(torch.uint8))
            c_el = dot_vec.double().repeat_interleave(2, dim=1)[:, None].abs()
            d_bound = ((E + D * 2.0 ** -24 * y.abs()) * c_el).sum(-1).permute(0, 2, 1) + 1e-7
            assert ((dot_out.double() - dots64).abs() <= d_bound).all()
    # the LSE of a forward on rotated, smoothed operands, restored, against the unrotated, unsmoothed bf16 forward: (1, 320, 4 / 2, D)
    g = torch.Generator().manual_seed(D)
    xq, xk, v = (torch.randn(1, 320, h, D, generator=g).bfloat16().cuda() for h in (4, 2, 2))
    tables = L.rope_tables(smooth.grid_for(320), D, device="cuda")
    args_q, args_k = (xq, wq, 1e-6, tables, norm), (xk, wk, 1e-6, tables, norm)
    q8, k8, dq, dk, lse_shift = L.SmoothedQK().pair(xq, xk, wq, wk, 1e-6, tables, norm, rotate=rot)
    v8, dv = L.E4m3Scales()(v, norm=None)
    _, lse8 = L.flash_attn_func(q8, k8, v8, q_descale=dq, k_descale=dk, v_descale=dv, return_softmax_lse=True)
    _, lse = L.flash_attn_func(L.qk_prep(*args_q), L.qk_prep(*args_k), v, return_softmax_lse=True)
    l_err = (L.lse_unshift(lse8, lse_shift, D ** -0.5) - lse).abs().max().item()
    print(f"D {D} {form}: max |LSE error| {l_err:.4f}")
    assert l_err <= 0.084


@pytest.mark.parametrize("D", [128, 64])
@pytest.mark.parametrize("concentrated,factor", [(True, 0.5), (False, 1.1)])
def test_dense_e4m3_attention_through_rotated_operands(D, concentrated, factor):
    """Rms error of O of the dense e4m3 forward, (1, 512, 2, D), against fp64 attention of the unquantized q, k, v. Two offset channels in
    q and k: the rotated error is at most half the plain one (measured: 6.9 x and 6.6 x lower). The offsets are twice those of the CPU
    simulation that motivated the feature: with those the first device run gave 2.17 x and 2.56 x, under 3 x - the error of O has a
    floor of 1.6e-3 from V and P in e4m3 - so the offset was made stronger, the factor kept. N(0, 1): no loss (1.1 x)."""
    import liteattention_amd as L
    g = torch.Generator().manual_seed(D)
    q, k, v = (torch.randn(1, 512, 2, D, generator=g) for _ in range(3))
    if concentrated:
        q[..., 5], k[..., 5], q[..., D - 3], k[..., D - 3] = q[..., 5] + 24, k[..., 5] + 40, q[..., D - 3] - 16, k[..., D - 3] + 30
    q, k, v = (t.bfloat16().cuda() for t in (q, k, v))
    scale = 1.0 / (8.0 * D ** 0.5)
    o64 = smooth._attention_fp64(q, k, v, scale)[0]
    v8, dv = L.E4m3Scales()(v, norm=None)
    errs = []
    for rot in (None, L.head_rotation(D, device="cuda")):
        (q8, dq), (k8, dk) = (L.E4m3Scales()(t, norm=None, rotate=rot) for t in (q, k))
        o = L.flash_attn_func(q8, k8, v8, softmax_scale=scale, q_descale=dq, k_descale=dk, v_descale=dv)
        errs.append((o.double() - o64).pow(2).mean().sqrt().item())
    print(f"D {D} concentrated {concentrated}: O rms error plain {errs[0]:.3e}, rotated {errs[1]:.3e}, ratio {errs[0] / errs[1]:.2f}x")
    assert errs[1] <= factor * errs[0]
