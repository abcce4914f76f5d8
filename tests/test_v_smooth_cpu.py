"""CPU: V smoothing (la_v_colstats, la_v_colstats_parts, la_v_colstats_part_rows, la_v_colstats_finish, la_attn_unshift) at the
boundary - the symbols, the argument structs, every validation rule in the order the header states (all of them answer before any HIP
call, so no device is needed) - and the host side: the fp64 references on hand-made inputs, v_shift_as_bias, the emulation the GPU
bounds are computed from, argument errors, the Meta ops."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import v_smooth_emulation as emu
from liteattention_amd import _cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lite_attention_amd.h")
NEW_SYMBOLS = ("la_v_colstats", "la_v_colstats_parts", "la_v_colstats_part_rows", "la_v_colstats_finish", "la_attn_unshift")


def test_the_entry_points_are_exported_declared_and_bound_under_abi_9():
    lib = _cabi.load()
    for name in NEW_SYMBOLS:
        assert name in _cabi.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.la_abi_version() == _cabi.LA_ABI_VERSION == 9
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+la_v_colstats\s*\(\s*const\s+la_v_colstats_args\s*\*", src)
    assert re.search(r"\bint\s+la_attn_unshift\s*\(\s*const\s+la_attn_unshift_args\s*\*", src)
    for fn in ("la_v_colstats_parts", "la_v_colstats_part_rows"):
        assert re.search(r"\bint\s+" + fn + r"\s*\(\s*int32_t\s+seqlen\s*,\s*int32_t\s+num_heads\s*,\s*int32_t\s+head_dim\s*\)", src)
    assert re.search(r"\bint\s+la_v_colstats_finish\s*\(\s*const\s+float\s*\*", src)
    assert lib.la_v_colstats.argtypes[0]._type_ is _cabi.LaVColstatsArgs
    assert lib.la_attn_unshift.argtypes[0]._type_ is _cabi.LaAttnUnshiftArgs
    out = subprocess.run(["nm", "-D", "--defined-only", _cabi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines()}
    assert set(NEW_SYMBOLS) <= exported
    import liteattention_amd
    import lite_attention
    for name in ("v_colstats", "v_colstats_parts", "v_colstats_reference", "attn_unshift", "attn_unshift_reference", "v_shift_as_bias",
                 "SmoothedV"):
        assert getattr(lite_attention, name) is getattr(liteattention_amd, name)
    assert hasattr(torch.ops.lite_attention, "v_colstats") and hasattr(torch.ops.lite_attention, "attn_unshift")


@pytest.mark.parametrize("c_name,mirror", [("la_v_colstats_args", _cabi.LaVColstatsArgs), ("la_attn_unshift_args", _cabi.LaAttnUnshiftArgs)])
def test_struct_layout_matches_header(tmp_path, c_name, mirror):
    """sizeof / offsetof as gcc compiles the header == the ctypes mirror; the older structs keep their sizes."""
    fields = [f[0] for f in mirror._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
            f'printf("%zu\\n", sizeof({c_name}));', 'printf("%zu\\n", sizeof(la_qk_prep_fp8_args));',
            'printf("%zu\\n", sizeof(la_qk_prep_smooth_args));']
    prog += [f'printf("%zu\\n", offsetof({c_name}, {f}));' for f in fields]
    prog += ["return 0;}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(exe), str(c)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(mirror)
    assert int(out[1]) == ctypes.sizeof(_cabi.LaQkPrepFp8Args) == 208 and int(out[2]) == ctypes.sizeof(_cabi.LaQkPrepSmoothArgs)
    for f, off in zip(fields, out[3:]):
        assert getattr(mirror, f).offset == int(off), f


# ---- la_v_colstats ---------------------------------------------------------------------------------------------------------------------
def _colstats_args(B=2, S=60, H=4, D=128, **changes):
    """Arguments that pass every check but the LAST one (the row stride is off 16 bytes): whatever is planted by `changes` in an earlier
    check must answer first, and no call ever reaches HIP. No pointer is dereferenced."""
    a = _cabi.LaVColstatsArgs()
    a.struct_size = ctypes.sizeof(_cabi.LaVColstatsArgs)
    a.in_dtype = _cabi.LA_DTYPE_BF16
    a.x, a.stat_part = 0x10000, 0x20000
    a.x_batch_stride, a.x_row_stride, a.x_head_stride = 3 * S * H * D, 3 * H * D + 4, D       # (the V slice of a fused projection)
    a.batch, a.seqlen, a.num_heads, a.head_dim = B, S, H, D
    for k, v in changes.items():
        setattr(a, k, v)
    return a


def _colstats_rc(**changes):
    return _cabi.load().la_v_colstats(ctypes.byref(_colstats_args(**changes)), None)


def test_colstats_errors_in_the_order_of_the_header():
    E = _cabi
    size = ctypes.sizeof(_cabi.LaVColstatsArgs)
    assert size == 64
    assert _colstats_rc() == E.LA_ERR_STRIDE                                               # the planted one, last in the order
    assert _cabi.load().la_v_colstats(None, None) == E.LA_ERR_NULL_ARG
    assert _colstats_rc(struct_size=size - 8, x=None) == E.LA_ERR_STRUCT_SIZE
    assert _colstats_rc(struct_size=size + 8, in_dtype=7) == E.LA_ERR_STRUCT_SIZE
    assert _colstats_rc(x=None, in_dtype=7) == E.LA_ERR_NULL_ARG
    assert _colstats_rc(stat_part=None, in_dtype=7) == E.LA_ERR_NULL_ARG
    assert _colstats_rc(in_dtype=7, seqlen=0) == E.LA_ERR_DTYPE
    assert _colstats_rc(in_dtype=E.LA_DTYPE_FP8_E4M3, seqlen=0) == E.LA_ERR_DTYPE
    for field in ("batch", "seqlen", "num_heads", "head_dim"):
        assert _colstats_rc(**{"head_dim": 100, field: 0}) == E.LA_ERR_SHAPE, field
        assert _colstats_rc(**{field: -3}) == E.LA_ERR_SHAPE, field
    assert _colstats_rc(head_dim=100) == E.LA_ERR_HEAD_DIM
    assert _colstats_rc(head_dim=264) == E.LA_ERR_HEAD_DIM                                 # % 8 == 0 but above 256
    assert _colstats_rc(head_dim=4) == E.LA_ERR_HEAD_DIM
    ok_rows = dict(x_row_stride=3 * 4 * 128)
    for field in ("x_batch_stride", "x_row_stride", "x_head_stride"):
        assert _colstats_rc(**{**ok_rows, field: -8}) == E.LA_ERR_STRIDE, field
    assert _colstats_rc(**ok_rows, x=0x10008) == E.LA_ERR_STRIDE                           # 16-byte loads
    assert _colstats_rc(**ok_rows, stat_part=0x20008) == E.LA_ERR_STRIDE                   # 16-byte stores
    assert _colstats_rc(**ok_rows, x_head_stride=132) == E.LA_ERR_STRIDE
    assert _colstats_rc(**ok_rows, x_batch_stride=60 * 4 * 128 + 4) == E.LA_ERR_STRIDE
    assert _colstats_rc(in_dtype=E.LA_DTYPE_FP32, x_head_stride=132, x_row_stride=4 * 132 + 2) == E.LA_ERR_STRIDE      # fp32: units of 4


def test_colstats_finish_rules():
    lib, E = _cabi.load(), _cabi
    ok = [0x10000, 8, 2, 4, 128, 60, 0x20000, 4 * 128, 128, 0x30000, 4, 1, None]
    names = ["part", "n_parts", "batch", "num_heads", "head_dim", "seqlen", "mean", "m_bs", "m_hs", "amax", "a_bs", "a_hs"]

    def rc(**ch):
        args = list(ok)
        for k, v in ch.items():
            args[names.index(k)] = v
        return lib.la_v_colstats_finish(*args)

    assert rc(part=None, n_parts=0) == E.LA_ERR_NULL_ARG and rc(mean=None, n_parts=0) == E.LA_ERR_NULL_ARG
    for k in ("n_parts", "batch", "num_heads", "head_dim", "seqlen"):
        assert rc(**{k: 0}, m_bs=-1) == E.LA_ERR_SHAPE, k
    assert rc(head_dim=264, m_bs=-1) == E.LA_ERR_HEAD_DIM
    for k in ("m_bs", "m_hs", "a_bs", "a_hs"):
        assert rc(**{k: -1}) == E.LA_ERR_STRIDE, k
    assert rc(part=0x10002) == E.LA_ERR_STRIDE and rc(mean=0x20001) == E.LA_ERR_STRIDE and rc(amax=0x30002) == E.LA_ERR_STRIDE


def test_parts_are_pure_and_cover_the_rows_exactly():
    lib = _cabi.load()
    import liteattention_amd as L
    seen = {}
    for _ in range(2):
        for S in (1, 63, 255, 256, 257, 600, 75600):
            for H, D in ((3, 64), (40, 128), (2, 256), (3, 40), (1, 8)):
                n, r = lib.la_v_colstats_parts(S, H, D), lib.la_v_colstats_part_rows(S, H, D)
                assert seen.setdefault((S, H, D), (n, r)) == (n, r)
                assert (n, r) == L.v_colstats_parts(S, H, D)
                assert n >= 1 and r >= 16 and n * r >= S and (n - 1) * r < S               # [0, S) exactly: no part without rows
                assert r == max(16, -(-S * H * (D // 8) // 131072))                        # the rule the header states
    assert seen[(75600, 40, 128)] == (205, 370) and seen[(600, 3, 64)] == (38, 16) and seen[(1, 3, 64)] == (1, 16)
    assert 205 * 40 * 16 >= 131072                                                         # the headline shape: one thread per slot
    for bad in ((0, 1, 8), (5, 0, 8), (5, 1, 0), (-1, 1, 8)):
        assert lib.la_v_colstats_parts(*bad) == _cabi.LA_ERR_SHAPE and lib.la_v_colstats_part_rows(*bad) == _cabi.LA_ERR_SHAPE
    with pytest.raises(ValueError):
        L.v_colstats_parts(0, 1, 8)


# ---- la_attn_unshift -------------------------------------------------------------------------------------------------------------------
def _unshift_args(B=2, S=60, H=4, D=128, **changes):
    """Valid but for the LAST check (lse_out off 4 bytes), everything asked for; out is the (B, S, H * D + 8) fp32 tensor."""
    a = _cabi.LaAttnUnshiftArgs()
    a.struct_size = ctypes.sizeof(_cabi.LaAttnUnshiftArgs)
    a.o_dtype, a.out_dtype, a.heads_per_vec = _cabi.LA_DTYPE_BF16, _cabi.LA_DTYPE_FP32, 2
    a.o, a.out, a.shift, a.lse, a.lse_dot, a.lse_out = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60002
    a.o_batch_stride, a.o_row_stride, a.o_head_stride = S * H * D, H * D, D
    a.out_batch_stride, a.out_row_stride, a.out_head_stride = S * (H * D + 8), H * D + 8, D
    a.batch, a.seqlen, a.num_heads, a.head_dim = B, S, H, D
    a.shift_batch_stride, a.shift_head_stride = H // 2 * D, D
    a.softmax_scale = D ** -0.5
    for k, v in changes.items():
        setattr(a, k, v)
    return a


def _unshift_rc(**changes):
    return _cabi.load().la_attn_unshift(ctypes.byref(_unshift_args(**changes)), None)


def test_unshift_errors_in_the_order_of_the_header():
    E = _cabi
    size = ctypes.sizeof(_cabi.LaAttnUnshiftArgs)
    PLANTED = E.LA_ERR_STRIDE
    assert _unshift_rc() == PLANTED
    assert _cabi.load().la_attn_unshift(None, None) == E.LA_ERR_NULL_ARG
    assert _unshift_rc(struct_size=size - 8, o=None) == E.LA_ERR_STRUCT_SIZE
    assert _unshift_rc(o=None, o_dtype=7) == E.LA_ERR_NULL_ARG
    assert _unshift_rc(out=None, o_dtype=7) == E.LA_ERR_NULL_ARG
    assert _unshift_rc(lse_dot=None, o_dtype=7) == E.LA_ERR_NULL_ARG                       # lse_out without lse_dot
    assert _unshift_rc(lse_out=None, o_dtype=7) == E.LA_ERR_NULL_ARG                       # lse_dot without lse_out
    assert _unshift_rc(lse=None, o_dtype=7) == E.LA_ERR_NULL_ARG                           # lse_dot without lse
    assert _unshift_rc(o_dtype=7, seqlen=0) == E.LA_ERR_DTYPE
    assert _unshift_rc(o_dtype=E.LA_DTYPE_FP32, seqlen=0) == E.LA_ERR_DTYPE                # o is what the forward returns: 16 bits
    assert _unshift_rc(out_dtype=E.LA_DTYPE_FP8_E4M3, seqlen=0) == E.LA_ERR_DTYPE
    for field in ("batch", "seqlen", "num_heads", "head_dim"):
        assert _unshift_rc(**{field: 0}, o_row_stride=-8) == E.LA_ERR_SHAPE, field
    assert _unshift_rc(heads_per_vec=3, head_dim=100) == E.LA_ERR_SHAPE                    # not a divisor of 4 heads
    assert _unshift_rc(heads_per_vec=0, head_dim=100) == E.LA_ERR_SHAPE
    assert _unshift_rc(heads_per_vec=0, shift=None) == PLANTED                             # ... only read with a shift
    assert _unshift_rc(head_dim=100, o_row_stride=-8) == E.LA_ERR_HEAD_DIM
    good = dict(lse_out=0x60000)                                                           # from here on nothing is planted: each line breaks
    for field in ("o_batch_stride", "o_row_stride", "o_head_stride", "out_batch_stride", "out_row_stride", "out_head_stride",
                  "shift_batch_stride", "shift_head_stride"):                              # one rule of the last group
        assert _unshift_rc(**good, **{field: -8}) == E.LA_ERR_STRIDE, field
    for field, ptr in (("o", 0x10008), ("out", 0x20008), ("shift", 0x30008), ("lse", 0x40002), ("lse_dot", 0x50001)):
        assert _unshift_rc(**good, **{field: ptr}) == E.LA_ERR_STRIDE, field
    assert _unshift_rc(**good, o_head_stride=132) == E.LA_ERR_STRIDE                       # 16-bit rows: units of 8 elements
    assert _unshift_rc(**good, out_row_stride=4 * 128 + 2) == E.LA_ERR_STRIDE              # fp32 rows: units of 4
    assert _unshift_rc(**good, out_dtype=E.LA_DTYPE_FP16, out_row_stride=4 * 128 + 4) == E.LA_ERR_STRIDE      # ... 16-bit out: of 8
    assert _unshift_rc(**good, shift_head_stride=130) == E.LA_ERR_STRIDE
    assert _unshift_rc(**good, shift_batch_stride=2 * 128 + 2) == E.LA_ERR_STRIDE
    # what is not used is free (the planted pointer answers)
    assert _unshift_rc(shift_head_stride=130, heads_per_vec=4) == PLANTED                  # one kv head: its stride is unused
    assert _unshift_rc(shift_batch_stride=2, o_batch_stride=3, out_batch_stride=1, batch=1) == PLANTED
    assert _unshift_rc(shift_head_stride=0, shift_batch_stride=0) == PLANTED               # a broadcast shift is a stride of 0


# ---- the references ------------------------------------------------------------------------------------------------------------------
def test_colstats_reference_on_a_hand_made_input():
    import liteattention_amd as L
    x = torch.zeros(1, 4, 2, 8)
    x[0, :, 0, 0] = torch.tensor([1.0, 2.0, 3.0, 6.0])            # mean 3: |x - mean| at most 3
    x[0, :, 0, 5] = torch.tensor([-1.0, -1.0, -1.0, -1.0])        # a pure offset: centred to 0
    x[0, :, 1, 7] = torch.tensor([0.0, 0.0, 0.0, -8.0])           # mean -2: |x - mean| at most 6
    mean, amax = L.v_colstats_reference(x.bfloat16())
    assert mean.dtype == amax.dtype == torch.float64 and mean.shape == (1, 2, 8) and amax.shape == (1, 2)
    want = torch.zeros(1, 2, 8, dtype=torch.float64)
    want[0, 0, 0], want[0, 0, 5], want[0, 1, 7] = 3.0, -1.0, -2.0
    assert torch.equal(mean, want) and amax.tolist() == [[3.0, 6.0]]
    x[0, 2, 1, 3] = float("nan")
    mean, amax = L.v_colstats_reference(x)
    assert mean[0, 1, 3].isnan() and mean.isnan().sum() == 1 and amax[0, 1].isnan() and not amax[0, 0].isnan()


def test_unshift_reference_on_a_hand_made_input_with_empty_rows():
    import liteattention_amd as L
    o = torch.arange(2 * 3 * 4 * 8, dtype=torch.float32).reshape(2, 3, 4, 8).bfloat16()
    shift = torch.arange(2 * 2 * 8, dtype=torch.float32).reshape(2, 2, 8) * 0.25
    got = L.attn_unshift_reference(o, shift)
    assert got.dtype == torch.float64
    for b in range(2):
        for h in range(4):
            assert torch.equal(got[b, :, h], o[b, :, h].double() + shift[b, h // 2].double())      # GQA: two q-heads per shift row
    assert torch.equal(L.attn_unshift_reference(o), o.double())                                     # no shift: the cast alone
    lse = torch.zeros(2, 4, 3)
    lse[0, 1, 2], lse[1, 3, 0], lse[1, 0, 1] = float("inf"), float("-inf"), float("nan")
    dot = torch.full((2, 4, 3), 2.0)
    out, lse_out = L.attn_unshift_reference(o, shift, lse=lse, lse_dot=dot, softmax_scale=0.5)
    assert out[0, 2, 1].abs().max() == 0 and out[1, 0, 3].abs().max() == 0                          # +inf and -inf rows: zeros
    assert lse_out[0, 1, 2] == float("inf") and lse_out[1, 3, 0] == float("-inf")                   # ... and their lse as it was
    assert torch.equal(out[1, 1, 0], got[1, 1, 0]) and lse_out[1, 0, 1].isnan()                     # a NaN row: the normal path
    mask = lse.isinf()
    assert torch.equal(lse_out[~mask & ~lse.isnan()], torch.full((21,), 1.0, dtype=torch.float64))  # 0 + 0.5 * 2
    keep = ~mask.transpose(1, 2)[..., None].expand_as(out)
    assert torch.equal(out[keep], got[keep])
    with pytest.raises(ValueError):
        L.attn_unshift_reference(o, shift, lse_dot=dot)                                             # lse_dot needs lse
    with pytest.raises(ValueError):
        L.attn_unshift_reference(o, torch.zeros(2, 3, 8))                                           # 3 kv heads for 4 q heads


def test_the_identity_the_feature_rests_on_in_fp64():
    """P (V - 1 m^T) + 1 m^T = P V for rows of P that sum to 1 - dense, over a subset of the keys, and after an LSE merge of two halves."""
    torch.manual_seed(11)
    q, k, v = (torch.randn(1, 40, 2, 16, dtype=torch.float64) for _ in range(3))
    v = v + 5.0
    m = v.mean(dim=1)

    def attention(kk, vv):
        s = torch.einsum("bqhd,bkhd->bhqk", q, kk) * 0.25
        return torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), vv), torch.logsumexp(s, -1)

    def merge(parts):
        lse = torch.logsumexp(torch.stack([l for _, l in parts]), 0)
        return sum(o * torch.exp(l - lse).transpose(1, 2)[..., None] for o, l in parts)

    o, _ = attention(k, v)
    o_shifted, _ = attention(k, v - m[:, None])
    assert torch.allclose(o_shifted + m[:, None], o, rtol=0, atol=1e-12)
    sub = torch.arange(40) % 3 != 0                                                    # a skip list: some keys never visited
    assert torch.allclose(attention(k[:, sub], (v - m[:, None])[:, sub])[0] + m[:, None], attention(k[:, sub], v[:, sub])[0], rtol=0, atol=1e-12)
    halves = [attention(k[:, :17], (v - m[:, None])[:, :17]), attention(k[:, 17:], (v - m[:, None])[:, 17:])]
    assert torch.allclose(merge(halves) + m[:, None], o, rtol=0, atol=1e-12)           # one shift for both halves: restore after the merge
    m2 = m + 1.0                                                                       # shifts that differ: restore BEFORE the merge
    parts = [attention(k[:, :17], (v - m[:, None])[:, :17]), attention(k[:, 17:], (v - m2[:, None])[:, 17:])]
    restored = [(parts[0][0] + m[:, None], parts[0][1]), (parts[1][0] + m2[:, None], parts[1][1])]
    assert torch.allclose(merge(restored), o, rtol=0, atol=1e-12)
    assert (merge(parts) + m[:, None] - o).abs().max() > 0.1


def test_v_shift_as_bias_against_the_explicit_add_in_fp64():
    import liteattention_amd as L
    torch.manual_seed(2)
    Hq, Hkv, D, F = 4, 2, 16, 24
    o = torch.randn(1, 10, Hq, D, dtype=torch.float64)
    w, b = torch.randn(F, Hq * D, dtype=torch.float64), torch.randn(F, dtype=torch.float64)
    shift = torch.randn(1, Hkv, D, dtype=torch.float64) * 4
    want = torch.nn.functional.linear((o + shift.repeat_interleave(Hq // Hkv, dim=1)[:, None]).flatten(2), w, b)
    bias = L.v_shift_as_bias(w, b, shift)
    assert bias.dtype == torch.float64 and bias.shape == (F,)
    assert torch.allclose(torch.nn.functional.linear(o.flatten(2), w, bias), want, rtol=0, atol=1e-11)
    assert torch.allclose(torch.nn.functional.linear(o.flatten(2), w, L.v_shift_as_bias(w, None, shift[0])), want - b, rtol=0, atol=1e-11)
    assert L.v_shift_as_bias(w.bfloat16(), b.bfloat16(), shift.float()).dtype == torch.float32      # never rounded to 16 bits unasked
    assert L.v_shift_as_bias(w.bfloat16(), None, shift.float(), dtype=torch.bfloat16).dtype == torch.bfloat16
    with pytest.raises(ValueError, match="per-batch"):
        L.v_shift_as_bias(w, b, shift.expand(2, Hkv, D))
    with pytest.raises(ValueError):
        L.v_shift_as_bias(w, b, torch.zeros(3, D, dtype=torch.float64))


# ---- the emulation the GPU bounds are computed from ---------------------------------------------------------------------------------
FORMS = ((False, False), (True, False), (True, True))          # (round_p, rowsum_of_rounded_p): P in fp32, rounded, rounded with its own sums


def test_emulation_ratios_at_offsets_0_and_16_lie_in_their_recorded_ranges():
    """Relative rms error of O against fp64, smoothed / plain, over the three forms of P, to the digits the ranges are recorded with
    (the emulation rows of profiles/v_smooth.md): offset 0: 1.002 - 1.003 for both output types; offset 16: 0.58 - 0.65 (O handed on
    in bf16), 0.30 - 0.34 (in fp32)."""
    for dtype in (torch.bfloat16, torch.float32):
        for rp, rs in FORMS:
            r0 = emu.smoothing_ratio(0, dtype, rp, rs)[0]
            assert 1.002 <= round(r0, 3) <= 1.003, (dtype, rp, rs, r0)
    for rp, rs in FORMS:
        r16 = emu.smoothing_ratio(16, torch.bfloat16, rp, rs)[0]
        assert 0.58 <= round(r16, 2) <= 0.65, (rp, rs, r16)
        r16 = emu.smoothing_ratio(16, torch.float32, rp, rs)[0]
        assert 0.30 <= round(r16, 2) <= 0.34, (rp, rs, r16)


def test_the_gpu_bounds_are_met_by_the_reference_alone():
    """tests/test_gpu_v_smooth.py asks: device ratio < min(1, 1.25 x the emulation's ratio) at offset 16, < 1.10 at offset 0, for the
    default form of P (rounded, fp32 row sums of the unrounded P). The emulation itself passes both."""
    for dtype in (torch.bfloat16, torch.float32):
        r16 = emu.smoothing_ratio(16, dtype, True, False)[0]
        assert r16 < min(1.0, 1.25 * r16) and 1.25 * r16 < 1.0
        assert emu.smoothing_ratio(0, dtype, True, False)[0] < 1.10


def test_emulation_options_do_what_they_say():
    q, k, v, o64, _ = emu.case(16)
    a = emu.fp8_attention_emulation(q, k, v, smooth_v=True, round_p=False, out_dtype=torch.float32)
    b = emu.fp8_attention_emulation(q, k, v, smooth_v=True, round_p=True, out_dtype=torch.float32)
    c = emu.fp8_attention_emulation(q, k, v, smooth_v=True, round_p=True, rowsum_of_rounded_p=True, out_dtype=torch.float32)
    assert a.dtype == torch.float32 and not torch.equal(a, b) and not torch.equal(b, c)
    assert emu.fp8_attention_emulation(q, k, v).dtype == torch.bfloat16
    assert emu.rel_rms(a, o64) < 0.01


# ---- argument errors, Meta ops -----------------------------------------------------------------------------------------------------------
def test_the_functions_refuse_cpu_tensors_and_bad_arguments():
    import liteattention_amd as L
    x = torch.zeros(1, 4, 4, 16, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="GPU"):
        L.v_colstats(x)
    with pytest.raises(ValueError, match="GPU"):
        L.attn_unshift(x, torch.zeros(1, 2, 16))
    with pytest.raises(ValueError, match="GPU"):
        L.SmoothedV()(x)
    with pytest.raises(ValueError):
        L.v_colstats(torch.zeros(4, 4, 16))
    with pytest.raises(ValueError):
        L.attn_unshift(x, torch.zeros(1, 3, 16))                                       # 3 kv heads for 4 q heads
    with pytest.raises(ValueError):
        L.attn_unshift(x, torch.zeros(1, 2, 16, dtype=torch.float64))
    with pytest.raises(ValueError):
        L.attn_unshift(x, lse_dot=torch.zeros(1, 4, 4))                                # lse_dot needs lse
    with pytest.raises(ValueError):
        L.attn_unshift(x, lse=torch.zeros(1, 4, 5))                                    # (B, H, S) = (1, 4, 4)
    with pytest.raises(ValueError):
        L.SmoothedV(mode="static")
    with pytest.raises(ValueError):
        L.SmoothedV(margin=0.0)
    with pytest.raises(ValueError):
        L.SmoothedV()(torch.zeros(4, 4, 16))
    with pytest.raises(RuntimeError):
        L.SmoothedV().finish(x)                                                        # no call yet: no shift


@pytest.mark.parametrize("cls", ["LiteAttention", "SeqParallelLiteAttention"])
def test_the_attention_classes_check_the_restoring_arguments_before_anything_runs(cls):
    import liteattention_amd as L
    q = torch.zeros(1, 64, 4, 128, dtype=torch.float8_e4m3fn)
    k = v = torch.zeros(1, 64, 2, 128, dtype=torch.float8_e4m3fn)
    if cls == "LiteAttention":
        la = L.LiteAttention(enable_skipping=False)
        call = lambda **kw: la(q, k, v, **kw)                                          # noqa: E731
    else:
        sp = L.SeqParallelLiteAttention(2, enable_skipping=False)
        call = lambda **kw: sp(q, k, v, 1, **kw)                                       # noqa: E731
    with pytest.raises(ValueError, match="v_shift"):
        call(v_shift=torch.zeros(1, 4, 128))                                           # per q-head: must be per kv-head
    with pytest.raises(ValueError, match="v_shift"):
        call(v_shift=torch.zeros(1, 2, 128, dtype=torch.float64))
    with pytest.raises(ValueError, match="v_shift"):
        call(v_shift=torch.zeros(2, 128))
    with pytest.raises(ValueError, match="lse_shift"):
        call(lse_shift=torch.zeros(1, 64, 4))                                          # (B, S, H): must be (B, H, S)
    with pytest.raises(ValueError, match="out_dtype"):
        call(out_dtype=torch.float64)


def test_meta_ops_give_shape_and_dtype_only():
    x = torch.empty(2, 60, 4, 128, dtype=torch.bfloat16, device="meta")
    mean, amax = torch.ops.lite_attention.v_colstats(x)
    assert mean.shape == (2, 4, 128) and amax.shape == (2, 4) and mean.dtype == amax.dtype == torch.float32 and mean.device.type == "meta"
    got = torch.ops.lite_attention.attn_unshift(x)
    assert got.shape == x.shape and got.dtype == torch.bfloat16 and got.device.type == "meta"
    got = torch.ops.lite_attention.attn_unshift(x, None, None, None, None, None, torch.float32)
    assert got.shape == x.shape and got.dtype == torch.float32
