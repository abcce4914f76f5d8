"""CPU: la_attn_unshift_fp8 / attn_out_fp8 (O restored and row-scaled to e4m3 in one pass) at the boundary - the symbol, the argument
struct, every validation rule in the order the header states (all of them answer before any HIP call, so no device is needed) - and
the host side: the fp64 reference against the fp32 emulation the GPU tests expect, typed argument errors, the Meta op, the checks of
the attention classes."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import attn_out_fp8_emulation as emu
from liteattention_amd import _cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lite_attention_amd.h")
F8 = torch.float8_e4m3fn


def test_the_entry_point_is_exported_declared_and_bound_under_abi_9():
    lib = _cabi.load()
    assert "la_attn_unshift_fp8" in _cabi.EXPORTED_SYMBOLS and hasattr(lib, "la_attn_unshift_fp8")
    assert lib.la_abi_version() == _cabi.LA_ABI_VERSION == 9
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+la_attn_unshift_fp8\s*\(\s*const\s+la_attn_unshift_fp8_args\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)", src)
    assert lib.la_attn_unshift_fp8.argtypes[0]._type_ is _cabi.LaAttnUnshiftFp8Args
    out = subprocess.run(["nm", "-D", "--defined-only", _cabi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "la_attn_unshift_fp8" in {ln.split()[-1] for ln in out.splitlines()}
    import liteattention_amd
    import lite_attention
    for name in ("attn_out_fp8", "attn_out_fp8_reference", "RowScaledE4m3"):
        assert name in liteattention_amd.__all__ and getattr(lite_attention, name) is getattr(liteattention_amd, name)
    assert hasattr(torch.ops.lite_attention, "attn_out_fp8")


def test_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof as gcc compiles the header == the ctypes mirror; la_attn_unshift_args keeps its size."""
    mirror, c_name = _cabi.LaAttnUnshiftFp8Args, "la_attn_unshift_fp8_args"
    fields = [f[0] for f in mirror._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
            f'printf("%zu\\n", sizeof({c_name}));', 'printf("%zu\\n", sizeof(la_attn_unshift_args));']
    prog += [f'printf("%zu\\n", offsetof({c_name}, {f}));' for f in fields]
    prog += ["return 0;}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(exe), str(c)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(mirror) == 216
    assert int(out[1]) == ctypes.sizeof(_cabi.LaAttnUnshiftArgs) == 152
    for f, off in zip(fields, out[2:]):
        assert getattr(mirror, f).offset == int(off), f
    assert len(fields) == len(set(fields)) == 32 and "out_dtype" not in fields


# ---- the validation rules ----------------------------------------------------------------------------------------------------------------
def _args(B=0x7fffffff, S=60, H=4, D=128, **changes):
    """Arguments that pass every check but the LAST one (2^31 - 1 batches of two tiles each: more workgroups than a grid has), everything
    asked for: shift of two kv heads, lse / lse_dot / lse_out, the dynamic mode with a padded row_descale, out a view of a (B, S, H * D
    + 8) buffer. Whatever is planted by `changes` in an earlier check must answer first, and no call ever reaches HIP: no pointer is
    dereferenced."""
    a = _cabi.LaAttnUnshiftFp8Args()
    a.struct_size = ctypes.sizeof(_cabi.LaAttnUnshiftFp8Args)
    a.o_dtype, a.heads_per_vec, a.heads_per_scale = _cabi.LA_DTYPE_BF16, 2, 2
    a.o, a.out, a.shift, a.lse, a.lse_dot, a.lse_out = 0x10000, 0x20008, 0x30000, 0x40000, 0x50000, 0x60000
    a.o_batch_stride, a.o_row_stride, a.o_head_stride = S * H * D, H * D, D
    a.out_batch_stride, a.out_row_stride, a.out_head_stride = S * (H * D + 8), H * D + 8, D
    a.batch, a.seqlen, a.num_heads, a.head_dim = B, S, H, D
    a.shift_batch_stride, a.shift_head_stride = H // 2 * D, D
    a.softmax_scale = D ** -0.5
    a.row_descale, a.row_descale_batch_stride, a.row_descale_row_stride, a.row_descale_group_stride = 0x70000, S * 3, 3, 1
    for k, v in changes.items():
        setattr(a, k, v)
    return a


def _rc(**changes):
    return _cabi.load().la_attn_unshift_fp8(ctypes.byref(_args(**changes)), None)


def test_errors_in_the_order_of_the_header():
    E = _cabi
    size = ctypes.sizeof(_cabi.LaAttnUnshiftFp8Args)
    PLANTED = E.LA_ERR_SHAPE                                                       # the last check: one workgroup per tile
    assert _rc() == PLANTED
    assert _cabi.load().la_attn_unshift_fp8(None, None) == E.LA_ERR_NULL_ARG
    assert _rc(struct_size=size - 8, o=None) == E.LA_ERR_STRUCT_SIZE
    assert _rc(struct_size=ctypes.sizeof(_cabi.LaAttnUnshiftArgs), o=None) == E.LA_ERR_STRUCT_SIZE     # la_attn_unshift's struct
    for field in ("o", "out", "row_descale", "lse_dot", "lse_out", "lse"):          # row_descale: the dynamic mode writes it
        assert _rc(**{field: None}, o_dtype=7) == E.LA_ERR_NULL_ARG, field
    assert _rc(row_descale=None, descale_in=0x80000) == PLANTED                    # ... the static mode does not
    assert _rc(o_dtype=7, seqlen=0) == E.LA_ERR_DTYPE
    assert _rc(o_dtype=E.LA_DTYPE_FP32, seqlen=0) == E.LA_ERR_DTYPE
    assert _rc(o_dtype=E.LA_DTYPE_FP8_E4M3, seqlen=0) == E.LA_ERR_DTYPE
    for field in ("batch", "seqlen", "num_heads", "head_dim"):
        assert _rc(**{field: 0}, o_row_stride=-8) == E.LA_ERR_SHAPE, field
        assert _rc(**{field: -2}, o_row_stride=-8) == E.LA_ERR_SHAPE, field
    head = dict(head_dim=100, batch=2)                                             # nothing planted at the end: SHAPE is the rule's own
    assert _rc(**head) == E.LA_ERR_HEAD_DIM
    assert _rc(**head, heads_per_vec=3) == E.LA_ERR_SHAPE                          # not a divisor of 4 heads
    assert _rc(**head, heads_per_vec=0) == E.LA_ERR_SHAPE
    assert _rc(**head, heads_per_vec=0, shift=None) == E.LA_ERR_HEAD_DIM           # ... only read with a shift
    for hps in (3, 0, -1, 8):
        assert _rc(**head, heads_per_scale=hps) == E.LA_ERR_SHAPE, hps             # hps does not divide H
    # a group of 256 * 128 elements is refused BEHIND the strides (LA_ERR_UNSUPPORTED): each line below breaks one rule of theirs
    bad_group = dict(batch=2, out=0x20000, num_heads=256, heads_per_scale=256)
    for field in ("o_batch_stride", "o_row_stride", "o_head_stride", "out_batch_stride", "out_row_stride", "out_head_stride",
                  "shift_batch_stride", "shift_head_stride", "row_descale_batch_stride", "row_descale_row_stride",
                  "row_descale_group_stride", "descale_in_batch_stride", "amax_batch_stride"):
        assert _rc(**bad_group, **{field: -8}) == E.LA_ERR_STRIDE, field
    for field, ptr in (("o", 0x10008), ("out", 0x20004), ("shift", 0x30008), ("lse", 0x40002), ("lse_dot", 0x50001), ("lse_out", 0x60002),
                       ("row_descale", 0x70002), ("descale_in", 0x80001), ("amax", 0x90002)):
        assert _rc(**{**bad_group, field: ptr}) == E.LA_ERR_STRIDE, field
    assert _rc(**bad_group, o_head_stride=132) == E.LA_ERR_STRIDE                  # 16-bit rows: units of 8 elements
    assert _rc(**bad_group, out_row_stride=256 * 128 + 4) == E.LA_ERR_STRIDE       # e4m3 rows: 8-byte stores
    assert _rc(**bad_group, out_head_stride=132) == E.LA_ERR_STRIDE
    assert _rc(**bad_group, out_batch_stride=60 * 256 * 128 + 4) == E.LA_ERR_STRIDE
    assert _rc(**bad_group, shift_head_stride=130) == E.LA_ERR_STRIDE
    assert _rc(**bad_group) == E.LA_ERR_UNSUPPORTED
    # behind the strides, in front of the grid: no in-place form, the group a wave holds, the heads a workgroup flags
    assert _rc(out=0x10000) == E.LA_ERR_UNSUPPORTED                                # out == o
    assert _rc(num_heads=256, heads_per_scale=256, heads_per_vec=128) == E.LA_ERR_UNSUPPORTED      # 32768 elements a group
    assert _rc(num_heads=128, heads_per_scale=128, heads_per_vec=64) == PLANTED                    # 16384: the limit itself
    assert _rc(num_heads=64, heads_per_scale=64, head_dim=264, heads_per_vec=32) == E.LA_ERR_UNSUPPORTED       # 16896
    assert _rc(num_heads=1032, heads_per_scale=1, heads_per_vec=1) == E.LA_ERR_UNSUPPORTED         # more than 1024 heads
    assert _rc(num_heads=1024, heads_per_scale=1, heads_per_vec=1) == PLANTED
    # what is not used is free (the planted end answers)
    assert _rc(shift_head_stride=130, heads_per_vec=4) == PLANTED                  # one kv head: its stride is unused
    assert _rc(shift_head_stride=0, shift_batch_stride=0) == PLANTED               # a broadcast shift is a stride of 0
    assert _rc(descale_in=0x80000, amax=0x90000, descale_in_batch_stride=0, amax_batch_stride=1) == PLANTED
    assert _rc(batch=0x7fffffff, seqlen=33) == PLANTED                             # two tiles a batch again


def test_la_attn_unshift_still_refuses_an_e4m3_out_dtype():
    a = _cabi.LaAttnUnshiftArgs()
    a.struct_size = ctypes.sizeof(_cabi.LaAttnUnshiftArgs)
    a.o_dtype, a.out_dtype, a.heads_per_vec = _cabi.LA_DTYPE_BF16, _cabi.LA_DTYPE_FP8_E4M3, 1
    a.o, a.out = 0x10000, 0x20000
    a.o_batch_stride = a.out_batch_stride = 60 * 512
    a.o_row_stride = a.out_row_stride = 512
    a.o_head_stride = a.out_head_stride = 128
    a.batch, a.seqlen, a.num_heads, a.head_dim = 1, 60, 4, 128
    assert _cabi.load().la_attn_unshift(ctypes.byref(a), None) == _cabi.LA_ERR_DTYPE


# ---- the reference and the emulation ------------------------------------------------------------------------------------------------------
def test_reference_and_emulation_agree_on_hand_made_rows():
    """Values chosen so that every fp32 step is exact: the fp64 reference and the fp32 emulation must then agree to the bit, and the
    bytes are the ones worked out by hand."""
    import liteattention_amd as L
    o = torch.zeros(1, 3, 2, 8)
    o[0, 0, 0] = torch.tensor([1.0, -2.0, 3.5, 0.0, 0.25, -0.125, 7.0, -7.0])     # amax 7 ... with the shift: 8
    o[0, 0, 1] = torch.tensor([0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5])
    o[0, 1, 1, 3] = -14.0                                                         # row 1: one value, negative, beside the shift
    o[0, 2, :, 6] = -1.0                                                          # row 2: the shift cancels it, y = 0
    shift = torch.zeros(1, 1, 8)
    shift[0, 0, 6] = 1.0                                                          # 7 + 1 = 8 is the largest |y| of row 0
    o = o.bfloat16()
    (z, d) = L.attn_out_fp8_reference(o, shift)
    data, de, y = emu.emulate(o, shift)
    assert z.dtype == d.dtype == torch.float64 and z.shape == (1, 3, 2, 8) and d.shape == (1, 3, 1)
    assert data.dtype == F8 and de.dtype == torch.float32 and de.shape == (1, 3, 1)
    assert d[0, :, 0].tolist() == [8.0 / 448, 14.0 / 448, 2.0 ** -100 / 448]
    assert torch.equal(de.double(), d.float().double())                           # the emulation's descale: the reference's, rounded once
    # (row, head, element): the scaled value, its e4m3 code (-392 lies between -384 and -416)
    want = {(0, 0, 6): (448.0, 448.0), (0, 0, 7): (-392.0, -384.0), (0, 1, 0): (28.0, 28.0), (1, 1, 3): (-448.0, -448.0),
            (1, 0, 6): (32.0, 32.0), (2, 1, 6): (0.0, 0.0)}
    for (s_, h_, j_), (z_, code) in want.items():
        assert abs(z[0, s_, h_, j_].item() - z_) < 1e-9 and data[0, s_, h_, j_].float() == code, (s_, h_, j_)
    assert data[0, 0, 0, 6].float() == 448.0 and data[0, 2].view(torch.uint8).eq(0).all()
    # per head: two groups a row
    (z1, d1) = L.attn_out_fp8_reference(o, shift, heads_per_scale=1)
    data1, de1, _ = emu.emulate(o, shift, heads_per_scale=1)
    assert d1.shape == (1, 3, 2) and d1[0, 0].tolist() == [8.0 / 448, 1.5 / 448] and z1[0, 0, 1, 6] == 448.0
    assert data1[0, 0, 1, 6].float() == 448.0 and data1[0, 0, 1, 0].float() == 144.0      # 149.33: between 144 and 160
    # the emulation against the reference within half an e4m3 step on random rows of nine decades
    g = torch.Generator().manual_seed(5)
    o = (torch.randn(2, 67, 5, 96, generator=g) * torch.exp2(torch.randint(-15, 15, (2, 67, 1, 1), generator=g).float())).bfloat16()
    shift = torch.randn(2, 5, 96, generator=g) * 0.01
    for hps in (1, 5):
        (z, d) = L.attn_out_fp8_reference(o, shift, heads_per_scale=hps)
        data, de, y = emu.emulate(o, shift, heads_per_scale=hps)
        y64 = L.attn_unshift_reference(o, shift)
        dd = de.double().repeat_interleave(hps, dim=2)[..., None]
        bound = torch.maximum(y64.abs() * 2.0 ** -4, dd * 2.0 ** -10) * (1 + 2.0 ** -16)
        err = (data.double() * dd - y64).abs()
        assert (err <= bound).all(), (err / bound).max().item()
        assert ((de.double() - d).abs() <= d * 2.0 ** -22).all()


def test_reference_rules_empty_rows_nan_static_and_lse():
    import liteattention_amd as L
    g = torch.Generator().manual_seed(3)
    o = torch.randn(2, 5, 4, 16, generator=g).bfloat16()
    shift = torch.randn(2, 2, 16, generator=g)
    lse = torch.zeros(2, 4, 5)
    lse[0, 1, 2], lse[0, 3, 2] = float("inf"), float("-inf")
    lse[1, :, 4] = float("inf")
    lse[1, 0, 0] = float("nan")
    (z, d) = L.attn_out_fp8_reference(o, shift, lse=lse)
    y = L.attn_unshift_reference(o, shift, lse=lse)
    assert z[0, 2, 1].abs().max() == 0 and z[0, 2, 3].abs().max() == 0
    assert d[0, 2, 0] == y[0, 2, [0, 2]].abs().max() / 448                          # the token's scale comes from the remaining heads
    assert d[1, 4, 0] == 2.0 ** -100 / 448 and z[1, 4].abs().max() == 0            # every head empty
    assert not z.isnan().any()                                                     # a NaN lse: the normal path
    dot = torch.full((2, 4, 5), 2.0)
    ((z2, d2), lse_out) = L.attn_out_fp8_reference(o, shift, lse=lse, lse_dot=dot, softmax_scale=0.5)
    assert torch.equal(z2, z) and torch.equal(d2, d)
    want = L.attn_unshift_reference(o, shift, lse=lse, lse_dot=dot, softmax_scale=0.5)[1]
    assert lse_out[1, 0, 0].isnan() and torch.equal(lse_out.nan_to_num(7.0), want.nan_to_num(7.0))
    on = o.clone()
    on[1, 3, 2, 5] = float("nan")
    (zn, dn) = L.attn_out_fp8_reference(on, shift, heads_per_scale=2)
    assert dn.isnan().sum() == 1 and dn[1, 3, 1].isnan() and zn[1, 3, 2:].isnan().all() and zn.isnan().sum() == 32
    en, edn, _ = emu.emulate(on, shift, heads_per_scale=2)
    assert edn.isnan().sum() == 1 and edn[1, 3, 1].isnan() and (en[1, 3, 2:].view(torch.uint8) & 0x7f).eq(0x7f).all()
    assert en.float().isnan().sum() == 32
    ds = torch.tensor([0.5, 0.001])
    (zs, dss) = L.attn_out_fp8_reference(o, shift, descale=ds)
    assert dss.shape == (2, 1, 1) and torch.equal(zs[0], L.attn_unshift_reference(o, shift)[0] / 0.5)
    assert zs[1].abs().max() == 448.0                                              # a scale too small: saturated, not wrapped
    es, _, _ = emu.emulate(o, shift, descale=ds)
    assert es[1].float().abs().max() == 448.0 and not es.float().isnan().any()
    (z1, d1) = L.attn_out_fp8_reference(o, shift, descale=torch.tensor([0.5]))
    assert torch.equal(z1[0], zs[0]) and d1.shape == (2, 1, 1)


# ---- argument errors, Meta op, the classes -----------------------------------------------------------------------------------------------
def test_typed_errors_before_any_launch():
    import liteattention_amd as L
    o = torch.zeros(1, 4, 4, 16, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="GPU"):
        L.attn_out_fp8(o)
    with pytest.raises(ValueError, match="heads_per_scale"):
        L.attn_out_fp8(o, heads_per_scale=3)
    with pytest.raises(ValueError, match="heads_per_scale"):
        L.attn_out_fp8(o, heads_per_scale=0)
    with pytest.raises(NotImplementedError, match="16384"):
        L.attn_out_fp8(torch.zeros(1, 2, 128, 256, dtype=torch.bfloat16))          # one scale per token of 32768 elements
    with pytest.raises(NotImplementedError, match="16384"):
        L.attn_out_fp8_reference(torch.zeros(1, 2, 128, 256, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        L.attn_out_fp8(o, torch.zeros(1, 3, 16))                                   # 3 kv heads for 4 q heads
    with pytest.raises(ValueError):
        L.attn_out_fp8(o, lse_dot=torch.zeros(1, 4, 4))                            # lse_dot needs lse
    with pytest.raises(ValueError, match="descale"):
        L.attn_out_fp8(o, descale=torch.zeros(3))                                  # B or 1 elements
    with pytest.raises(ValueError, match="descale"):
        L.attn_out_fp8(o, descale=torch.zeros(1, dtype=torch.float64))
    with pytest.raises(ValueError, match="amax_out"):
        L.attn_out_fp8(o, amax_out=torch.zeros(1))                                 # the running maximum belongs to the static mode
    with pytest.raises(ValueError, match="amax_out"):
        L.attn_out_fp8(o, descale=torch.ones(1), amax_out=torch.zeros(2))
    with pytest.raises(ValueError, match="head_dim"):
        L.attn_out_fp8(torch.zeros(1, 4, 4, 12, dtype=torch.bfloat16))
    sv = L.SmoothedV()
    with pytest.raises(RuntimeError):
        sv.finish(o, fp8=True)                                                     # no call yet: no shift
    sv.shift = torch.zeros(1, 2, 16)
    with pytest.raises(ValueError, match="out_dtype"):
        sv.finish(o, fp8=True, out_dtype=torch.float32)
    with pytest.raises(ValueError, match="fp8=True"):
        sv.finish(o, heads_per_scale=2)
    with pytest.raises(ValueError, match="heads_per_scale"):
        sv.finish(o, fp8=True, heads_per_scale=3)
    with pytest.raises(ValueError, match="GPU"):
        sv.finish(o, fp8=True, heads_per_scale=2, out=torch.zeros(1, 4, 4, 16).to(F8))


def test_row_scaled_e4m3_as_matrix():
    import liteattention_amd as L
    data = torch.zeros(2, 5, 4, 16).to(F8)
    r = L.RowScaledE4m3(data, torch.ones(2, 5, 1))
    m, s = r.as_matrix()
    assert m.shape == (10, 64) and s.shape == (10, 1) and m.data_ptr() == data.data_ptr() and m.dtype == F8
    d2, s2 = r
    assert d2 is data and s2 is r.descale
    with pytest.raises(ValueError, match="one scale per token"):
        L.RowScaledE4m3(data, torch.ones(2, 5, 2)).as_matrix()
    with pytest.raises(ValueError, match="contiguous"):
        L.RowScaledE4m3(torch.zeros(2, 5, 4, 32).to(F8)[..., :16], torch.ones(2, 5, 1)).as_matrix()


def test_meta_op_gives_shape_and_dtype_only():
    x = torch.empty(2, 60, 4, 128, dtype=torch.bfloat16, device="meta")
    data, ds = torch.ops.lite_attention.attn_out_fp8(x)
    assert data.shape == x.shape and data.dtype == F8 and data.device.type == "meta"
    assert ds.shape == (2, 60, 1) and ds.dtype == torch.float32
    data, ds = torch.ops.lite_attention.attn_out_fp8(x, None, None, None, None, 2)
    assert ds.shape == (2, 60, 2)
    data, ds = torch.ops.lite_attention.attn_out_fp8(x, None, None, None, None, None, torch.empty(2, device="meta"))
    assert ds.shape == (2,) and data.shape == x.shape


@pytest.mark.parametrize("cls", ["LiteAttention", "SeqParallelLiteAttention"])
def test_the_attention_classes_check_out_fp8_before_anything_runs(cls):
    import liteattention_amd as L
    q = torch.zeros(1, 64, 4, 128, dtype=F8)
    k = v = torch.zeros(1, 64, 2, 128, dtype=F8)
    if cls == "LiteAttention":
        la = L.LiteAttention(enable_skipping=False)
        call = lambda **kw: la(q, k, v, **kw)                                          # noqa: E731
    else:
        sp = L.SeqParallelLiteAttention(2, enable_skipping=False)
        call = lambda **kw: sp(q, k, v, 1, **kw)                                       # noqa: E731
    with pytest.raises(ValueError, match="out_dtype"):
        call(out_fp8=True, out_dtype=torch.float32)
    with pytest.raises(ValueError, match="out_dtype"):
        call(out_fp8=dict(heads_per_scale=1), out_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="out_dtype"):
        call(out_dtype=torch.float64)                                                  # as before
    with pytest.raises(ValueError, match="heads_per_scale"):
        call(out_fp8=dict(heads_per_scale=3))
    with pytest.raises(ValueError, match="out_fp8"):
        call(out_fp8=dict(group=2))
    with pytest.raises(ValueError, match="out_fp8"):
        call(out_fp8="yes")
    with pytest.raises(ValueError, match="descale"):
        call(out_fp8=dict(descale=torch.zeros(3)))
    with pytest.raises(ValueError, match="v_shift"):
        call(out_fp8=True, v_shift=torch.zeros(1, 4, 128))                             # per q-head: must be per kv-head
