"""GPU: fp8 V in one pass (la_v_prep_tiles). The pass must write, byte for byte, the V^T tiles that the two passes it replaces write -
the quantizer `qk_prep_smooth(x, norm=None, ...)` and la_fwd's own prepare pass over its e4m3 result - and the forward fed the
resulting `PreparedV` must not be able to tell: O, LSE and every written skip list are bit-identical. Everything on the reference side
is code that existed before the pass did."""
import ctypes
import os
import sys

import pytest
import torch

from helpers import structured_qkv

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
pytestmark = pytest.mark.gpu
F8 = torch.float8_e4m3fn
HEAD_DIMS = (64, 96, 128, 192, 256)
GUARD, TAIL, FILL = 256, 512, 0xA5


def _x(B, S, Hk, D, dtype=torch.bfloat16, seed=0, fused=False):
    """V as a projection writes it: 3 + randn (a mean worth subtracting), bf16-representable; `fused`: the V slice of a (B, S, 3, H, D) one."""
    g = torch.Generator(device="cuda").manual_seed(1000 * D + 7 * S + seed)
    if fused:
        return (3.0 + torch.randn(B, S, 3, Hk, D, device="cuda", generator=g)).to(dtype)[:, :, 2]
    return (3.0 + torch.randn(B, S, Hk, D, device="cuda", generator=g)).to(dtype)


def _scales(B, Hk, D, seed=0, shift=True, descale=True):
    g = torch.Generator(device="cuda").manual_seed(seed + 5)
    sh = (3.0 + 0.1 * torch.randn(B, Hk, D, device="cuda", generator=g)) if shift else None
    ds = (0.004 + 0.01 * torch.rand(B, Hk, device="cuda", generator=g)) if descale else None       # 448 * descale: 1.8 .. 6.3
    return sh, ds


def _tiles_by_the_two_passes(x, shift, descale):
    """The reference side: the quantizing pass, then a raw dense la_fwd (Sq = 64) on a test-owned workspace prefilled with FILL; returns
    the first la_v_tiles_bytes of that workspace - what la_fwd's prepare pass wrote."""
    import liteattention_amd as L
    from liteattention_amd import _cabi
    from liteattention_amd import flash_attn_interface as fai
    B, S, Hk, D = x.shape
    v8 = L.qk_prep_smooth(x, norm=None, shift=shift, descale=descale)
    q = torch.zeros((B, 64, Hk, D), dtype=torch.uint8, device="cuda").view(F8)
    k = torch.zeros((B, S, Hk, D), dtype=torch.uint8, device="cuda").view(F8)
    out = torch.empty((B, 64, Hk, D), dtype=torch.bfloat16, device="cuda")
    lse = torch.empty((B, Hk, 64), dtype=torch.float32, device="cuda")
    bm, bn = _cabi.get_tile_sizes(D, 1)
    a = fai._fwd_args(q, k, v8, out, lse, (None, None, None), B, 64, S, D ** -0.5, bm, bn)
    lib = _cabi.load()
    need = lib.la_fwd_workspace_bytes(ctypes.byref(a))
    tiles, ws = L.v_tiles_bytes(B, Hk, S, D)
    assert need == ws
    work = torch.full((need,), FILL, dtype=torch.uint8, device="cuda")
    a.workspace, a.workspace_bytes = work.data_ptr(), need
    rc = lib.la_fwd(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _cabi.status_string(rc)
    torch.cuda.synchronize()
    return work[:tiles].clone(), v8


def _tiles_in_one_pass(x, shift, descale, amax_out=None):
    """`v_prep_tiles` into the middle of a FILL-ed buffer: (tile bytes, the PreparedV); guard, counters and tail must still be FILL."""
    import liteattention_amd as L
    B, S, Hk, D = x.shape
    tiles, ws = L.v_tiles_bytes(B, Hk, S, D)
    buf = torch.full((GUARD + ws + TAIL,), FILL, dtype=torch.uint8, device="cuda")
    pv = L.v_prep_tiles(x, descale=descale, shift=shift, amax_out=amax_out, out=buf[GUARD:])
    torch.cuda.synchronize()
    assert isinstance(pv, L.PreparedV) and pv.shape == x.shape and pv.descale is descale and pv.device == x.device
    assert bool((buf[:GUARD] == FILL).all()), "bytes in front of the tile region changed"
    assert bool((buf[GUARD + tiles:] == FILL).all()), "bytes behind the tile region changed"
    return buf[GUARD: GUARD + tiles].clone(), pv


def _check_same_tiles(x, shift, descale):
    want, _ = _tiles_by_the_two_passes(x, shift, descale)
    got, _ = _tiles_in_one_pass(x, shift, descale)
    assert want.numel() == got.numel() > 0
    diff = (want != got).nonzero()
    assert diff.numel() == 0, f"{diff.numel()} tile bytes differ, the first at {int(diff[0])}: {int(want[diff[0]])} vs {int(got[diff[0]])}"
    assert bool((got != FILL).any())                                                       # (the pass ran)


# ---- T1: the tile bytes are the prepare pass's -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("Sk", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("D", HEAD_DIMS)
def test_tile_bytes_equal_the_prepare_passes(D, Sk):
    B, Hk = 2, 2
    shift, descale = _scales(B, Hk, D)
    _check_same_tiles(_x(B, Sk, Hk, D), shift, descale)


@pytest.mark.parametrize("variant", ["fp16", "fp32", "fused", "shift_only", "descale_only", "neither"])
def test_tile_bytes_at_head_dim_128_other_inputs(variant):
    B, Sk, Hk, D = 2, 200, 2, 128
    dtype = {"fp16": torch.float16, "fp32": torch.float32}.get(variant, torch.bfloat16)
    x = _x(B, Sk, Hk, D, dtype, fused=variant == "fused")
    if variant == "fp32":
        x = x + 1e-4 * torch.randn_like(x)                                                 # off the bf16 grid
    if variant == "fused":
        assert not x.is_contiguous() and x.stride(1) == 3 * Hk * D
    shift, descale = _scales(B, Hk, D, shift=variant != "descale_only" and variant != "neither",
                             descale=variant != "shift_only" and variant != "neither")
    _check_same_tiles(x, shift, descale)


def test_tile_bytes_with_non_finite_and_saturating_values():
    B, Sk, Hk, D = 2, 200, 2, 128
    x = _x(B, Sk, Hk, D)
    shift, descale = _scales(B, Hk, D)
    x[0, 3, 0, 5], x[0, 70, 1, 127], x[1, 199, 0, 0] = float("nan"), float("inf"), float("-inf")
    x[1, 64, 1, 8:24] = 1000.0                                                             # beyond 448 * descale (at most 6.3) + shift
    x[0, 130, 1, 40:48] = -1000.0
    want, v8 = _tiles_by_the_two_passes(x, shift, descale)
    got, _ = _tiles_in_one_pass(x, shift, descale)
    assert torch.equal(want, got)
    codes = v8.view(torch.uint8)
    assert (int(codes[0, 3, 0, 5]) & 0x7F) == 0x7F and int(codes[0, 70, 1, 127]) == 0x7E and int(codes[1, 199, 0, 0]) == 0xFE
    assert bool((codes[1, 64, 1, 8:24] == 0x7E).all()) and bool((codes[0, 130, 1, 40:48] == 0xFE).all())


def test_reference_codes_equal_the_quantizers_on_finite_values():
    import liteattention_amd as L
    B, Sk, Hk, D = 2, 200, 2, 128
    x = _x(B, Sk, Hk, D)
    shift, descale = _scales(B, Hk, D)
    v8 = L.qk_prep_smooth(x, norm=None, shift=shift, descale=descale)
    assert torch.equal(L.v_prep_tiles_reference(x, shift=shift, descale=descale).view(torch.uint8), v8.view(torch.uint8))


# ---- T2: amax ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,Sk", [(128, 200), (96, 65), (256, 1)])
def test_amax_bits_equal_the_amax_pass(D, Sk):
    import liteattention_amd as L
    B, Hk = 2, 2
    x = _x(B, Sk, Hk, D)
    shift, descale = _scales(B, Hk, D)
    want = torch.zeros((B, Hk), device="cuda")
    L.qk_prep_smooth(x, norm=None, shift=shift, amax_out=want, quantize=False)
    got = torch.zeros((B, Hk), device="cuda")
    _tiles_in_one_pass(x, shift, descale, amax_out=got)
    assert torch.equal(want.view(torch.int32), got.view(torch.int32)) and bool((got > 0).all())
    # a larger value that is already there stays; a smaller one is raised
    pre = want.clone()
    pre[0, 0], pre[1, 1] = 1e6, 1e-3
    _tiles_in_one_pass(x, shift, descale, amax_out=pre)
    assert float(pre[0, 0]) == 1e6 and torch.equal(pre.flatten()[1:].view(torch.int32), want.flatten()[1:].view(torch.int32))


def test_a_nan_makes_its_heads_amax_nan_and_no_others():
    import liteattention_amd as L
    B, Sk, Hk, D = 2, 200, 2, 128
    x = _x(B, Sk, Hk, D)
    x[1, 150, 0, 77] = float("nan")
    shift, descale = _scales(B, Hk, D)
    want = torch.zeros((B, Hk), device="cuda")
    L.qk_prep_smooth(x, norm=None, shift=shift, amax_out=want, quantize=False)
    got = torch.zeros((B, Hk), device="cuda")
    _tiles_in_one_pass(x, shift, descale, amax_out=got)
    assert torch.equal(want.view(torch.int32), got.view(torch.int32))
    assert got.isnan().tolist() == [[False, False], [True, False]]


# ---- T3: determinism ---------------------------------------------------------------------------------------------------------------------
def test_two_launches_give_identical_bytes():
    B, Sk, Hk, D = 2, 200, 3, 192
    x = _x(B, Sk, Hk, D)
    shift, descale = _scales(B, Hk, D)
    am1, am2 = torch.zeros((B, Hk), device="cuda"), torch.zeros((B, Hk), device="cuda")
    t1, _ = _tiles_in_one_pass(x, shift, descale, amax_out=am1)
    t2, _ = _tiles_in_one_pass(x, shift, descale, amax_out=am2)
    assert torch.equal(t1, t2) and torch.equal(am1.view(torch.int32), am2.view(torch.int32))


def test_the_op_writes_the_same_workspace():
    import liteattention_amd as L
    B, Sk, Hk, D = 2, 200, 2, 128
    x = _x(B, Sk, Hk, D)
    shift, descale = _scales(B, Hk, D)
    tiles, ws = L.v_tiles_bytes(B, Hk, Sk, D)
    want = L.v_prep_tiles(x, shift=shift, descale=descale).workspace[:tiles]
    got = torch.ops.lite_attention.v_prep_tiles(x, descale, shift)
    assert got.dtype == torch.uint8 and got.numel() == ws and torch.equal(got[:tiles], want)
    mine = torch.zeros(ws + 64, dtype=torch.uint8, device="cuda")
    assert torch.ops.lite_attention.v_prep_tiles(x, descale, shift, None, mine).data_ptr() == mine.data_ptr()
    assert torch.equal(mine[:tiles], want)


@pytest.mark.parametrize("mode", ["current", "delayed"])
def test_e4m3_scales_with_tiles_over_steps(mode):
    """`E4m3Scales(tiles=True)` beside `E4m3Scales()` on a V that grows from step to step (delayed: the descale of step t is made from
    step t - 1's amax, collected by the tile pass itself): the same descales, and the same O from the attention call."""
    import liteattention_amd as L
    B, Sq, Sk, H, Hk, D = 1, 130, 200, 4, 2, 128
    g = torch.Generator(device="cuda").manual_seed(3)
    q = torch.randn(B, Sq, H, D, device="cuda", generator=g).to(F8)
    k = torch.randn(B, Sk, Hk, D, device="cuda", generator=g).to(F8)
    es_a, es_b = L.E4m3Scales(mode=mode, margin=1.25), L.E4m3Scales(mode=mode, margin=1.25, tiles=True)
    for step in range(3):
        x = _x(B, Sk, Hk, D, seed=step) * (1.0 + 0.2 * step)
        v8, dv_a = es_a(x, norm=None)
        pv, dv_b = es_b(x, norm=None)
        assert isinstance(pv, L.PreparedV) and pv.descale is dv_b and torch.equal(dv_a, dv_b), step
        assert torch.equal(es_a.amax.view(torch.int32), es_b.amax.view(torch.int32)), step
        o_a = L.flash_attn_func(q, k, v8, v_descale=dv_a)
        o_b = L.flash_attn_func(q, k, pv, v_descale=dv_b)
        assert torch.equal(o_a, o_b), step
    assert es_b.out is pv


# ---- T4: the forward cannot tell the difference --------------------------------------------------------------------------------------
def _no_workspace(*a, **k):
    raise AssertionError("a call with a PreparedV allocated a workspace of its own")


@pytest.mark.parametrize("D", HEAD_DIMS)
def test_dense_call_is_bit_identical(D, monkeypatch):
    import liteattention_amd as L
    from liteattention_amd import flash_attn_interface as fai
    B, Sq, Sk, H, Hk = 1, 130, 200, 4, 2
    g = torch.Generator(device="cuda").manual_seed(D)
    q = torch.randn(B, Sq, H, D, device="cuda", generator=g).to(F8)
    k = torch.randn(B, Sk, Hk, D, device="cuda", generator=g).to(F8)
    qd, kd = 0.5 + torch.rand(B, Hk, device="cuda", generator=g), 0.5 + torch.rand(B, Hk, device="cuda", generator=g)
    x = _x(B, Sk, Hk, D)
    shift, dv = _scales(B, Hk, D)
    v8 = L.qk_prep_smooth(x, norm=None, shift=shift, descale=dv)
    o_a, lse_a = L.flash_attn_func(q, k, v8, q_descale=qd, k_descale=kd, v_descale=dv, return_softmax_lse=True)
    pv = L.v_prep_tiles(x, shift=shift, descale=dv)
    monkeypatch.setattr(fai, "_add_workspace", _no_workspace)
    o_b, lse_b = L.flash_attn_func(q, k, pv, q_descale=qd, k_descale=kd, v_descale=dv, return_softmax_lse=True)
    assert o_b.dtype == torch.bfloat16 and torch.equal(o_a, o_b) and torch.equal(lse_a, lse_b)
    assert not o_a.float().isnan().any() and float(o_a.float().abs().max()) > 0
    # ... and once more on the same tiles: the call leaves them as they were
    o_c = L.flash_attn_func(q, k, pv, q_descale=qd, k_descale=kd, v_descale=dv)
    assert torch.equal(o_a, o_c)
    # a dense LiteAttention call: restored and cast like a tensor's, never split over the keys
    att = L.LiteAttention(enable_skipping=False)
    o_d = att(q, k, pv, q_descale=qd, k_descale=kd, v_descale=dv, v_shift=shift, out_dtype=torch.float32)
    assert torch.equal(o_d, L.attn_unshift(o_a, shift, out_dtype=torch.float32))


def _skipping_inputs():
    B, S, H = 1, 1536, 2
    q, k, v = structured_qkv(B, S, H, 128, seed=300, alpha=9.0, dtype=torch.float32)
    qd, kd = torch.tensor([[0.7, 1.3]]).cuda(), torch.tensor([[1.1, 0.9]]).cuda()
    return q.to(F8).cuda(), k.to(F8).cuda(), (3.0 + v).bfloat16().cuda(), qd, kd


def test_three_skipping_steps_with_smoothed_v_are_bit_identical(monkeypatch):
    """The structured inputs of the e4m3 list test, V through SmoothedV: tensor route and tile route side by side, O (restored, fp32),
    LSE and both ping-pong lists equal after every step - and the tensor route's third step does walk a shortened list."""
    import liteattention_amd as L
    from liteattention_amd import flash_attn_interface as fai
    q, k, xv, qd, kd = _skipping_inputs()
    att_a, att_b = (L.LiteAttention(threshold=-3.0, max_batch_size=1) for _ in range(2))
    sv_a, sv_b = L.SmoothedV(), L.SmoothedV(tiles=True)
    add_workspace = fai._add_workspace
    for step in range(3):
        v8, dv_a, sh_a = sv_a(xv)
        o_a, lse_a = att_a(q, k, v8, return_softmax_lse=True, q_descale=qd, k_descale=kd, v_descale=dv_a, v_shift=sh_a,
                           out_dtype=torch.float32)
        pv, dv_b, sh_b = sv_b(xv)
        assert isinstance(pv, L.PreparedV) and pv.descale is dv_b and torch.equal(dv_a, dv_b) and torch.equal(sh_a, sh_b)
        monkeypatch.setattr(fai, "_add_workspace", _no_workspace)
        o_b, lse_b = att_b(q, k, pv, return_softmax_lse=True, q_descale=qd, k_descale=kd, v_descale=dv_b, v_shift=sh_b,
                           out_dtype=torch.float32)
        monkeypatch.setattr(fai, "_add_workspace", add_workspace)
        assert o_b.dtype == torch.float32 and torch.equal(o_a, o_b) and torch.equal(lse_a, lse_b), step
        assert att_a._phase == att_b._phase and torch.equal(att_a._skip_list, att_b._skip_list), step
        if step == 1:
            assert att_a.get_skip_fraction(batch=1) > 0, "the third step of the tensor route reads a full list: nothing was tested"
    assert sv_b.v8 is pv                                                                   # the workspace of the first call, reused


def test_two_windows_are_bit_identical():
    import liteattention_amd as L
    q, k, xv, qd, kd = _skipping_inputs()
    shift, dv = _scales(1, 2, 128)
    v8 = L.qk_prep_smooth(xv, norm=None, shift=shift, descale=dv)
    pv = L.v_prep_tiles(xv, shift=shift, descale=dv)
    bm, _ = L.get_tile_sizes(128, 1)
    q_tiles = -(-q.shape[1] // bm)
    windows = [(0, q_tiles // 2), (q_tiles // 2, q_tiles - q_tiles // 2)]
    att_a, att_b = (L.LiteAttention(threshold=-3.0, max_batch_size=1) for _ in range(2))
    for step in range(2):
        o_a, lse_a = att_a.call_windowed(q, k, v8, windows, return_softmax_lse=True, q_descale=qd, k_descale=kd, v_descale=dv)
        o_b, lse_b = att_b.call_windowed(q, k, pv, windows, return_softmax_lse=True, q_descale=qd, k_descale=kd, v_descale=dv)
        assert torch.equal(o_a, o_b) and torch.equal(lse_a, lse_b) and torch.equal(att_a._skip_list, att_b._skip_list), step


# ---- T5: the demo ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smooth_v", [True, False])
def test_demo_rows_are_the_same_with_v_tiles(smooth_v):
    """640 tokens: at most 704 keys, where the demo's block with skipping disabled is not split over the keys with a tensor V either
    (a PreparedV is never split), so every row - skipped fraction and error against that block - must be EQUAL, not merely close."""
    import wan_self_attention_demo as demo
    kw = dict(frames=5, height=8, width=16, heads=2, steps=3, verbose=False, fp8=True, smooth_v=smooth_v)
    rows = demo.run(**kw, v_tiles=False)
    assert demo.run(**kw, v_tiles=True) == rows
    assert len(rows) == 3


# ---- T6: HIP graph -----------------------------------------------------------------------------------------------------------------------
def test_v_pass_and_attention_capture_and_replay():
    import liteattention_amd as L
    B, Sq, Sk, H, Hk, D = 1, 300, 200, 4, 2, 128
    g = torch.Generator(device="cuda").manual_seed(11)
    q = torch.randn(B, Sq, H, D, device="cuda", generator=g).to(F8)
    k = torch.randn(B, Sk, Hk, D, device="cuda", generator=g).to(F8)
    data = [_x(B, Sk, Hk, D, seed=s) for s in range(3)]
    sv = L.SmoothedV(tiles=True)

    def step(x):
        pv, dv, shift = sv(x)
        o, lse = L.flash_attn_func(q, k, pv, v_descale=dv, return_softmax_lse=True)
        return sv.finish(o, lse=lse, out_dtype=torch.float32), lse

    eager = [tuple(t.clone() for t in step(x)) for x in data]
    buf = data[0].clone()
    step(buf)                                                                              # warm-up: every buffer exists before the capture
    workspace = sv.v8.workspace
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o_g, lse_g = step(buf)
    assert sv.v8.workspace is workspace
    for x, (o, lse) in zip(data, eager):
        buf.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o_g, o) and torch.equal(lse_g, lse)
