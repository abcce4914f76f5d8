"""CPU: fp8 V in one pass (la_v_prep_tiles, la_v_tiles_bytes, la_v_tiles_workspace_bytes) at the boundary - the symbols, the argument
struct, every validation rule in the order the header states (all of them answer before any HIP call, so no device is needed), the two
size functions against la_fwd_workspace_bytes - and the host side: what a PreparedV refuses before anything is launched."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from liteattention_amd import _cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lite_attention_amd.h")
NEW_SYMBOLS = ("la_v_prep_tiles", "la_v_tiles_bytes", "la_v_tiles_workspace_bytes")
HEAD_DIMS = (64, 96, 128, 192, 256)
E4M3 = torch.float8_e4m3fn


def test_the_entry_points_are_exported_declared_bound_and_documented_under_abi_9():
    lib = _cabi.load()
    for name in NEW_SYMBOLS:
        assert name in _cabi.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.la_abi_version() == _cabi.LA_ABI_VERSION == 9
    header = open(HEADER).read()
    assert re.search(r"#define\s+LA_ABI_VERSION\s+9\b", header)
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+la_v_prep_tiles\s*\(\s*const\s+la_v_prep_tiles_args\s*\*", src)
    for fn in ("la_v_tiles_bytes", "la_v_tiles_workspace_bytes"):
        assert re.search(r"\bint64_t\s+" + fn + r"\s*\(\s*int32_t\s+batch\s*,\s*int32_t\s+num_heads_k\s*,\s*int32_t\s+seqlen_k\s*,"
                         r"\s*int32_t\s+head_dim\s*\)", src)
        assert getattr(lib, fn).restype is ctypes.c_int64
    assert lib.la_v_prep_tiles.argtypes[0]._type_ is _cabi.LaVPrepTilesArgs
    out = subprocess.run(["nm", "-D", "--defined-only", _cabi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert set(NEW_SYMBOLS) <= {ln.split()[-1] for ln in out.splitlines()}
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    top = header[: header.index("#ifndef LITE_ATTENTION_AMD_H")]
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\b", integration), name
        assert re.search(r"\b" + name + r"\b", top), name
    import liteattention_amd
    import lite_attention
    for name in ("v_prep_tiles", "v_prep_tiles_reference", "v_tiles_bytes", "PreparedV"):
        assert getattr(lite_attention, name) is getattr(liteattention_amd, name)
    assert hasattr(torch.ops.lite_attention, "v_prep_tiles")


def test_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof as gcc compiles the header == the ctypes mirror; the older structs keep their sizes."""
    mirror = _cabi.LaVPrepTilesArgs
    fields = [f[0] for f in mirror._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
            'printf("%zu\\n", sizeof(la_v_prep_tiles_args));', 'printf("%zu\\n", sizeof(la_fwd_args));',
            'printf("%zu\\n", sizeof(la_qk_prep_smooth_args));']
    prog += [f'printf("%zu\\n", offsetof(la_v_prep_tiles_args, {f}));' for f in fields]
    prog += ["return 0;}"]
    c = tmp_path / "layout.c"
    c.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(exe), str(c)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert int(out[0]) == ctypes.sizeof(mirror) == 144
    assert int(out[1]) == ctypes.sizeof(_cabi.LaFwdArgs) and int(out[2]) == ctypes.sizeof(_cabi.LaQkPrepSmoothArgs)
    for f, off in zip(fields, out[3:]):
        assert getattr(mirror, f).offset == int(off), f


# ---- la_v_prep_tiles: the order of the checks ------------------------------------------------------------------------------------------
def _args(**changes):
    """Arguments that pass every check but the LAST one (2^15 * 2^15 * 2 tiles are more than one grid holds): whatever `changes` plants
    in an earlier check must answer first, and no call ever reaches HIP. No pointer is dereferenced."""
    B, S, H, D = 1 << 15, 128, 1 << 15, 128
    a = _cabi.LaVPrepTilesArgs()
    a.struct_size = ctypes.sizeof(_cabi.LaVPrepTilesArgs)
    a.in_dtype = _cabi.LA_DTYPE_BF16
    a.x, a.tiles = 0x10000, 0x20000
    a.x_batch_stride, a.x_row_stride, a.x_head_stride = 3 * S * H * D, 3 * H * D, D       # (the V slice of a fused projection)
    a.batch, a.seqlen, a.num_heads, a.head_dim = B, S, H, D
    a.descale, a.descale_batch_stride, a.descale_head_stride = 0x30000, H, 1
    a.shift, a.shift_batch_stride, a.shift_head_stride = 0x40000, H * D, D
    a.amax, a.amax_batch_stride, a.amax_head_stride = 0x50000, H, 1
    for k, v in changes.items():
        setattr(a, k, v)
    return a


def _rc(**changes):
    return _cabi.load().la_v_prep_tiles(ctypes.byref(_args(**changes)), None)


def test_errors_in_the_order_of_the_header():
    E = _cabi
    size = ctypes.sizeof(_cabi.LaVPrepTilesArgs)
    assert _rc() == E.LA_ERR_SHAPE                                                         # the planted one, last in the order
    assert _rc(seqlen=65) == E.LA_ERR_SHAPE                                                # (tiles, not rows: 65 rows are two)
    assert _cabi.load().la_v_prep_tiles(None, None) == E.LA_ERR_NULL_ARG
    assert _rc(struct_size=size - 8, x=None) == E.LA_ERR_STRUCT_SIZE
    assert _rc(struct_size=size + 8, in_dtype=7) == E.LA_ERR_STRUCT_SIZE
    assert _rc(x=None, in_dtype=7) == E.LA_ERR_NULL_ARG
    assert _rc(tiles=None, in_dtype=7) == E.LA_ERR_NULL_ARG
    assert _rc(in_dtype=7, seqlen=0) == E.LA_ERR_DTYPE
    assert _rc(in_dtype=E.LA_DTYPE_FP8_E4M3, seqlen=0) == E.LA_ERR_DTYPE
    for field in ("batch", "seqlen", "num_heads", "head_dim"):
        assert _rc(**{"head_dim": 100, field: 0}) == E.LA_ERR_SHAPE, field
        assert _rc(**{"head_dim": 100, field: -3}) == E.LA_ERR_SHAPE, field
    assert _rc(head_dim=100, reserved0=1) == E.LA_ERR_HEAD_DIM
    assert _rc(reserved0=1, x=0x10008) == E.LA_ERR_UNSUPPORTED
    for field in ("x_batch_stride", "x_row_stride", "x_head_stride", "descale_batch_stride", "descale_head_stride", "shift_batch_stride",
                  "shift_head_stride", "amax_batch_stride", "amax_head_stride"):
        assert _rc(**{field: -8}) == E.LA_ERR_STRIDE, field
    assert _rc(x=0x10008) == E.LA_ERR_STRIDE                                               # 16-byte loads
    assert _rc(tiles=0x20008) == E.LA_ERR_STRIDE                                           # 16-byte stores
    assert _rc(shift=0x40008) == E.LA_ERR_STRIDE
    assert _rc(shift_head_stride=130) == E.LA_ERR_STRIDE
    assert _rc(descale=0x30002) == E.LA_ERR_STRIDE and _rc(amax=0x50002) == E.LA_ERR_STRIDE
    assert _rc(x_head_stride=132) == E.LA_ERR_STRIDE
    assert _rc(in_dtype=E.LA_DTYPE_FP32, x_head_stride=130) == E.LA_ERR_STRIDE             # fp32: units of 4
    assert _rc(in_dtype=E.LA_DTYPE_FP32, x_head_stride=132) == E.LA_ERR_SHAPE              # ... which 132 is: on to the planted one
    # the optional pointers are optional: without them the same walk ends at the planted check
    assert _rc(descale=None, shift=None, amax=None) == E.LA_ERR_SHAPE
    assert _rc(shift=None, shift_head_stride=130) == E.LA_ERR_SHAPE


@pytest.mark.parametrize("head_dim", [0, -64, 8, 16, 32, 48, 72, 80, 100, 112, 120, 136, 160, 224, 264, 320, 512])
def test_every_other_head_dim_is_refused(head_dim):
    lib = _cabi.load()
    if head_dim > 0:
        assert _rc(head_dim=head_dim) == _cabi.LA_ERR_HEAD_DIM
    else:
        assert _rc(head_dim=head_dim) == _cabi.LA_ERR_SHAPE
    assert lib.la_v_tiles_bytes(2, 2, 100, head_dim) == _cabi.LA_ERR_HEAD_DIM
    assert lib.la_v_tiles_workspace_bytes(2, 2, 100, head_dim) == _cabi.LA_ERR_HEAD_DIM


def test_the_five_head_dims_pass_the_head_dim_check():
    for D in HEAD_DIMS:
        assert _rc(head_dim=D, x_head_stride=D, x_row_stride=(1 << 15) * D, shift_head_stride=D) == _cabi.LA_ERR_SHAPE     # the planted one


# ---- the size functions ----------------------------------------------------------------------------------------------------------------
GRID = [(B, Hk, S, D) for B in (1, 3) for Hk in (1, 5) for S in (1, 63, 64, 65, 200, 4096, 75600) for D in HEAD_DIMS]


def test_tile_bytes_formula():
    lib = _cabi.load()
    for B, Hk, S, D in GRID:
        assert lib.la_v_tiles_bytes(B, Hk, S, D) == B * Hk * -(-S // 64) * 64 * (128 if D == 96 else D), (B, Hk, S, D)
        assert lib.la_v_tiles_workspace_bytes(B, Hk, S, D) > lib.la_v_tiles_bytes(B, Hk, S, D)
    assert lib.la_v_tiles_bytes(1, 40, 75600, 128) == 40 * 1182 * 64 * 128
    assert lib.la_v_tiles_bytes(1, 1, 0, 128) == 0                                         # no keys: la_fwd takes them, so do the sizes
    for bad in ((0, 1, 64, 128), (1, 0, 64, 128), (1, 1, -1, 128), (-2, 1, 64, 128)):
        assert lib.la_v_tiles_bytes(*bad) == _cabi.LA_ERR_SHAPE and lib.la_v_tiles_workspace_bytes(*bad) == _cabi.LA_ERR_SHAPE


def _fwd_args(B, Hk, S, D, lists, flags, h_ratio=2, seqlen_q=300):
    a = _cabi.LaFwdArgs()
    a.struct_size = ctypes.sizeof(_cabi.LaFwdArgs)
    a.dtype = _cabi.LA_DTYPE_FP8_E4M3
    a.batch, a.seqlen_q, a.seqlen_k, a.num_heads, a.num_heads_k, a.head_dim, a.head_dim_v = B, seqlen_q, S, Hk * h_ratio, Hk, D, D
    a.flags = flags
    if lists:
        a.read_list, a.write_list = 0x10000, 0x20000
    return a


@pytest.mark.parametrize("lists", [False, True])
@pytest.mark.parametrize("flags", [0, _cabi.LA_FLAG_STATIC_SCHED, _cabi.LA_FLAG_V_PREPARED, _cabi.LA_FLAG_V_PREPARED | _cabi.LA_FLAG_STATIC_SCHED])
def test_the_workspace_serves_every_unsplit_fixed_length_fp8_launch(lists, flags):
    """Up to the 1182 key tiles of the headline shape no head dim cuts a dense launch into runs (about 1 600 tiles fit at head dims 192 /
    256, about 4 800 below): what la_fwd asks for is what la_v_tiles_workspace_bytes gives - not merely at most that."""
    lib = _cabi.load()
    for B, Hk, S, D in GRID:
        need = lib.la_fwd_workspace_bytes(ctypes.byref(_fwd_args(B, Hk, S, D, lists, flags)))
        assert 0 < need == lib.la_v_tiles_workspace_bytes(B, Hk, S, D), (B, Hk, S, D)


def test_keys_cut_into_runs_are_the_documented_exception():
    """Far enough out every head dim cuts a dense la_fwd into runs (the tiles of ONE run plus the partials: another size; under
    LA_FLAG_V_PREPARED la_fwd refuses such a launch). A launch with lists is never cut and still fits."""
    lib = _cabi.load()
    for D in HEAD_DIMS:
        S = 75600
        while lib.la_fwd_workspace_bytes(ctypes.byref(_fwd_args(1, 2, S, D, False, 0))) == lib.la_v_tiles_workspace_bytes(1, 2, S, D):
            S *= 2
            assert S < 1 << 24, D
        assert lib.la_fwd_workspace_bytes(ctypes.byref(_fwd_args(1, 2, S, D, True, 0))) == lib.la_v_tiles_workspace_bytes(1, 2, S, D)


# ---- PreparedV: what is refused before any launch --------------------------------------------------------------------------------------
def _prepared(B=2, Sk=200, Hk=2, D=128):
    from liteattention_amd import PreparedV, v_tiles_bytes
    tiles, ws = v_tiles_bytes(B, Hk, Sk, D)
    assert ws == tiles + 1024
    return PreparedV(torch.zeros(ws, dtype=torch.uint8), (B, Sk, Hk, D))


def _qk(B=2, Sq=130, Sk=200, H=4, Hk=2, D=128, dtype=E4M3):
    return torch.zeros((B, Sq, H, D)).to(dtype), torch.zeros((B, Sk, Hk, D)).to(dtype)


def test_prepared_v_holds_what_the_issue_says():
    pv = _prepared()
    assert pv.workspace.dtype == torch.uint8 and tuple(pv.shape) == (2, 200, 2, 128) and pv.device == torch.device("cpu")
    assert pv.descale is None
    v = pv.as_v()
    assert v.dtype == E4M3 and tuple(v.shape) == (2, 200, 2, 128) and v.data_ptr() == pv.workspace.data_ptr() and v.is_contiguous()


def test_prepared_v_constructor_refusals():
    from liteattention_amd import PreparedV, v_tiles_bytes
    ws = v_tiles_bytes(2, 2, 200, 128)[1]
    buf = torch.zeros(ws + 16, dtype=torch.uint8)
    with pytest.raises(ValueError, match="at least"):
        PreparedV(buf[: ws - 1], (2, 200, 2, 128))
    with pytest.raises(ValueError, match="uint8"):
        PreparedV(torch.zeros(ws, dtype=torch.int8), (2, 200, 2, 128))
    with pytest.raises(ValueError, match="16-byte"):
        PreparedV(buf[8: 8 + ws], (2, 200, 2, 128))
    with pytest.raises(ValueError, match="non-empty"):
        PreparedV(buf, (2, 0, 2, 128))
    for D in (80, 112, 160):                                                               # would run zero-padded
        with pytest.raises(NotImplementedError, match="zero-padded"):
            PreparedV(torch.zeros(1 << 20, dtype=torch.uint8), (2, 200, 2, D))


def _entry_points(pv):
    """The three ways in, as callables of (q, k, **kw)."""
    from liteattention_amd import LiteAttention, flash_attn_func
    return (("flash_attn_func", lambda q, k, **kw: flash_attn_func(q, k, pv, **kw)),
            ("LiteAttention", lambda q, k, **kw: LiteAttention(enable_skipping=False)(q, k, pv, **kw)),
            ("call_windowed", lambda q, k, **kw: LiteAttention(enable_skipping=False).call_windowed(q, k, pv, [(0, 1)], **kw)))


def test_prepared_v_call_refusals_need_no_device():
    pv = _prepared()
    for name, call in _entry_points(pv):
        q, k = _qk(dtype=torch.bfloat16)
        with pytest.raises(ValueError, match="float8_e4m3fn"):                             # q or k not e4m3
            call(q, k)
        q8, k8 = _qk()
        with pytest.raises(ValueError, match="float8_e4m3fn"):
            call(q8, k)
        for bad in (dict(Sk=199), dict(Hk=1), dict(Hk=4), dict(D=64), dict(B=1)):          # shapes, kv-head count, head_dim, batch
            q, k = _qk(**bad)
            with pytest.raises(ValueError, match="was made for"):
                call(q, k)
        q, k = _qk()
        with pytest.raises(ValueError, match="lives on"):
            call(q.to("meta"), k.to("meta"))
        with pytest.raises(NotImplementedError, match="fixed-length"):                     # packed: 3-D tensors
            call(q[0], k[0])
    q, k = _qk()
    from liteattention_amd import flash_attn_func
    from liteattention_amd.flash_attn_interface import mha_fwd
    for n in (2, 4, -1):
        with pytest.raises(NotImplementedError, match="split-KV"):
            flash_attn_func(q, k, pv, num_splits=n)
        with pytest.raises(NotImplementedError, match="split-KV"):
            mha_fwd(q, k, pv.as_v(), num_splits=n, _v_prepared=pv)
    cu = torch.tensor([0, 130, 260], dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="fixed-length"):
        mha_fwd(q, k, pv.as_v(), cu_seqlens_q=cu, cu_seqlens_k=cu, max_seqlen_q=130, max_seqlen_k=200, _v_prepared=pv)
    with pytest.raises(TypeError, match="PreparedV"):
        flash_attn_func(q, k, None)
    # ... and what passes them reaches the forward, which has no CPU path
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        flash_attn_func(q, k, pv)


def test_a_dense_lite_attention_call_with_a_prepared_v_asks_for_no_split(monkeypatch):
    """The dense call of a tensor V passes num_splits=-1 to flash_attn_func; with a PreparedV nothing asks for a split: mha_fwd gets
    the PreparedV, its view, the lists of the call and no num_splits."""
    import liteattention_amd.flash_attn_interface as fai
    from liteattention_amd import LiteAttention
    seen = {}

    def fake(q, k, v, **kw):
        seen.update(kw, v=v)
        return torch.zeros(q.shape, dtype=torch.bfloat16), torch.zeros((q.shape[0], q.shape[2], q.shape[1])), None, None

    monkeypatch.setattr(fai, "mha_fwd", fake)
    pv = _prepared()
    q, k = _qk()
    dv = torch.ones((2, 2))
    out = LiteAttention(enable_skipping=False)(q, k, pv, v_descale=dv)
    assert tuple(out.shape) == tuple(q.shape)
    assert "num_splits" not in seen and seen["_v_prepared"] is pv and seen["v"].data_ptr() == pv.workspace.data_ptr()
    assert seen["attn_read_list"] is None and seen["v_descale"] is dv and seen["q_descale"] is None


def test_tiles_switches_of_the_scale_objects():
    from liteattention_amd import E4m3Scales, SmoothedV
    assert SmoothedV().tiles is False and SmoothedV(tiles=True).tiles is True
    assert E4m3Scales().tiles is False and E4m3Scales(tiles=True).tiles is True
    with pytest.raises(ValueError, match="heads_per_scale"):
        E4m3Scales(tiles=True, heads_per_scale=2)
    x = torch.zeros((1, 8, 2, 128), dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="norm=None"):
        E4m3Scales(tiles=True)(x)                                                          # the default norm is "token"
    with pytest.raises(ValueError, match="norm=None"):
        E4m3Scales(tiles=True)(x, torch.ones(256), norm=None)


def test_reference_codes_on_hand_made_values():
    from liteattention_amd import v_prep_tiles_reference
    x = torch.tensor([0.0, 1.0, -2.0, 448.0, 1000.0, -1000.0, float("inf"), float("-inf")]).view(1, 1, 1, 8)
    codes = v_prep_tiles_reference(x).view(torch.uint8).flatten().tolist()
    assert codes == [0x00, 0x38, 0xC0, 0x7E, 0x7E, 0xFE, 0x7E, 0xFE]
    shifted = v_prep_tiles_reference(x[..., :3], descale=torch.tensor([[0.5]]), shift=torch.tensor([[[1.0, 1.0, 1.0]]]))
    assert shifted.float().flatten().tolist() == [-2.0, 0.0, -6.0]
    assert v_prep_tiles_reference(torch.tensor([float("nan")]).view(1, 1, 1, 1)).float().isnan().all()


def test_meta_op():
    x = torch.empty((2, 200, 2, 128), dtype=torch.bfloat16, device="meta")
    out = torch.ops.lite_attention.v_prep_tiles(x)
    assert out.dtype == torch.uint8 and out.numel() == _cabi.load().la_v_tiles_workspace_bytes(2, 2, 200, 128)
