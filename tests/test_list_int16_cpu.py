"""CPU: int16 skip lists (LA_FLAG_LIST_INT16, ABI 9) - the host layer and the argument checks of the C-ABI. Nothing here launches:
every C call below fails (or is refused) before any HIP call, and the attention call of ``LiteAttention`` is replaced by a recorder."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import liteattention_amd as L
from liteattention_amd import _cabi
from liteattention_amd import flash_attn_interface as fai
from liteattention_amd import lite_attention as la_mod
from liteattention_amd import skip_lists as sl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, q, k, v, softmax_scale=None, attn_read_list=None, attn_must_do_list=None,
                 attn_write_list=None, thr=None, return_softmax_lse=False, **kw):
        self.calls.append(dict(read=attn_read_list, write=attn_write_list, must_do=attn_must_do_list))
        return torch.zeros_like(q)


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(la_mod, "flash_attn_func", r)
    return r


def test_abi_9_and_the_flag_bit():
    assert _cabi.LA_ABI_VERSION == 9 and _cabi.load().la_abi_version() == 9
    assert _cabi.LA_FLAG_LIST_INT16 == 128
    assert _cabi.build_info()["abi"] == "9"
    assert not (_cabi.GEOMETRY_FLAGS & _cabi.LA_FLAG_LIST_INT16)          # the element type does not change the tiles


@pytest.mark.parametrize("must_skip", [None, [900, 600, 300, 100]])
def test_init_skip_list_int16_is_the_int32_list_cast(must_skip):
    args = (3, 1000, 2, 128, False, torch.bfloat16, "cpu")
    l32 = L.LiteAttention.init_skip_list(*args, must_skip_list=must_skip, seq_len_k=1500)
    l16 = L.LiteAttention.init_skip_list(*args, must_skip_list=must_skip, seq_len_k=1500, list_dtype=torch.int16)
    assert l32.dtype == torch.int32 and l16.dtype == torch.int16 and l16.shape == l32.shape
    assert torch.equal(l16, l32.to(torch.int16)) and torch.equal(l16.to(torch.int32), l32)
    assert l16.nbytes * 2 == l32.nbytes
    s16 = sl.new_skip_lists(1, 2, 3, 10, "cpu", list_dtype=torch.int16)
    assert s16.dtype == torch.int16 and torch.equal(s16.to(torch.int32), sl.new_skip_lists(1, 2, 3, 10, "cpu"))
    assert sl.listed_fraction(s16[0]) == sl.listed_fraction(s16[0].to(torch.int32)) == 1.0


def test_list_dtype_is_validated():
    with pytest.raises(ValueError):
        sl.new_skip_lists(1, 1, 1, 4, "cpu", list_dtype=torch.int64)
    with pytest.raises(ValueError):
        L.LiteAttention(list_dtype=torch.uint8)
    with pytest.raises(ValueError):                                        # a row of k_tiles + 1 = 32768 entries does not fit int16
        sl.check_list_dtype(torch.int16, 32767)
    assert sl.check_list_dtype(torch.int16, 32766) == torch.int16
    assert sl.check_list_dtype(torch.int32, 1 << 20) == torch.int32


def test_read_write_list_dtype_rule():
    """The helper mha_fwd and the varlen path call first: int32 or int16, one dtype for the pair; the reference's message otherwise."""
    i32, i16 = torch.zeros(1, 1, 1, 3, dtype=torch.int32), torch.zeros(1, 1, 1, 3, dtype=torch.int16)
    assert fai._list_flags(None, None) == 0
    assert fai._list_flags(i32, i32) == 0
    assert fai._list_flags(i16, i16) == _cabi.LA_FLAG_LIST_INT16
    for bad in (torch.int64, torch.uint8, torch.float32, torch.int8):
        t = torch.zeros(1, 1, 1, 3, dtype=bad)
        with pytest.raises(RuntimeError, match="attn_read_list must be int32 tensor"):
            fai._list_flags(t, i32)
        with pytest.raises(RuntimeError, match="attn_write_list must be int32 tensor"):
            fai._list_flags(i32, t)
    for rd, wr in ((i32, i16), (i16, i32)):
        with pytest.raises(RuntimeError, match="same dtype"):
            fai._list_flags(rd, wr)
    q = torch.zeros(1, 64, 1, 128, dtype=torch.bfloat16)
    assert fai._check_list(i16, "attn_read_list", q, fai.LIST_DTYPES) == i16.data_ptr()
    with pytest.raises(RuntimeError, match="attn_must_do_list must be int32 tensor"):      # the must-do list stays int32
        fai._check_list(i16, "attn_must_do_list", q)
    with pytest.raises(RuntimeError, match="contiguous int32 tensor"):
        fai.skip_list_stats(torch.zeros(1, 1, 1, 3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU implementation"):                       # int16 passes the dtype check
        fai.skip_list_stats(i16)


def _fwd_args(seqlen_k=256):
    a = _cabi.LaFwdArgs()
    a.struct_size = ctypes.sizeof(_cabi.LaFwdArgs)
    a.dtype = _cabi.LA_DTYPE_BF16
    a.q = a.k = a.v = a.o = 0x1000
    a.batch, a.seqlen_q, a.seqlen_k, a.num_heads, a.num_heads_k, a.head_dim, a.head_dim_v = 1, 256, seqlen_k, 4, 4, 128, 128
    a.block_m, a.block_n = 256, 64
    a.q_row_stride = a.k_row_stride = a.v_row_stride = a.o_row_stride = 4 * 128
    a.q_head_stride = a.k_head_stride = a.v_head_stride = a.o_head_stride = 128
    return a


def test_la_fwd_refuses_int16_rows_that_are_too_long_before_any_launch():
    lib = _cabi.load()
    for dtype in (_cabi.LA_DTYPE_BF16, _cabi.LA_DTYPE_FP16, _cabi.LA_DTYPE_FP8_E4M3):
        for extra in (0, _cabi.LA_FLAG_HALF_VOTE, _cabi.LA_FLAG_STATIC_SCHED):
            a = _fwd_args(seqlen_k=64 * 32767)                              # k_tiles + 1 = 32768
            a.dtype = dtype
            a.read_list, a.write_list = 0x2000, 0x3000
            a.flags = _cabi.LA_FLAG_LIST_INT16 | extra
            if extra == _cabi.LA_FLAG_HALF_VOTE and dtype != _cabi.LA_DTYPE_FP8_E4M3:
                a.block_m = 128
            if dtype == _cabi.LA_DTYPE_FP8_E4M3:                            # the workspace check comes first for e4m3: give one (never touched)
                a.workspace, a.workspace_bytes = 0x10000, 1 << 62
            assert lib.la_fwd(ctypes.byref(a), None) == _cabi.LA_ERR_SEQLEN, (dtype, extra)
    a = _fwd_args(seqlen_k=64 * 32767)
    a.flags = _cabi.LA_FLAG_LIST_INT16 | _cabi.LA_FLAG_KERNEL_128ROW
    a.block_m = 128
    a.read_list, a.write_list = 0x2000, 0x3000
    assert lib.la_fwd(ctypes.byref(a), None) == _cabi.LA_ERR_SEQLEN
    # the flag types the list pointers: without lists it means nothing; with one list only, the pair rule answers
    a = _fwd_args()
    a.flags = _cabi.LA_FLAG_LIST_INT16
    assert lib.la_fwd(ctypes.byref(a), None) == _cabi.LA_ERR_UNSUPPORTED
    a.read_list = 0x2000
    assert lib.la_fwd(ctypes.byref(a), None) == _cabi.LA_ERR_LISTS
    # the flag is known to the tile query and changes no tile
    m, n = ctypes.c_int(), ctypes.c_int()
    assert lib.la_get_tile_sizes_ex(128, 2, _cabi.LA_FLAG_LIST_INT16, ctypes.byref(m), ctypes.byref(n)) == 0 and (m.value, n.value) == (256, 64)
    a = _fwd_args()
    a.read_list, a.write_list = 0x2000, 0x3000
    a.flags = _cabi.LA_FLAG_LIST_INT16
    assert lib.la_fwd_workspace_bytes(ctypes.byref(a)) == 1024               # as for int32 lists


def test_ex_entry_points_validate_without_a_device():
    lib = _cabi.load()
    buf = (ctypes.c_int16 * 16)()
    out = (ctypes.c_int64 * 2)()
    m = (ctypes.c_uint8 * 16)()
    st, bm = lib.la_skip_list_stats_ex, lib.la_blockmask_to_lists_ex
    assert st(None, 2, 1, 1, 1, 1, out, None) == _cabi.LA_ERR_NULL_ARG
    assert st(buf, 2, 1, 1, 1, 1, None, None) == _cabi.LA_ERR_NULL_ARG
    for size in (0, 1, 3, 8, -2):
        assert st(buf, size, 1, 1, 1, 1, out, None) == _cabi.LA_ERR_DTYPE, size
    for shape in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)):
        assert st(buf, 2, *shape, out, None) == st(buf, 4, *shape, out, None) == _cabi.LA_ERR_SHAPE
    assert st(buf, 2, 1, 1, 1, 32767, out, None) == _cabi.LA_ERR_SEQLEN     # k_tiles + 1 = 32768 entries per row
    assert st(buf, 4, 1 << 20, 1 << 10, 1 << 10, 32767, out, None) == _cabi.LA_ERR_SHAPE   # (int32: no such bound; the row-count check answers)

    assert bm(None, 0, 0, 1, 1, 1, 1, None, None, buf, 2, None, None) == _cabi.LA_ERR_NULL_ARG
    assert bm(m, 0, 0, 1, 1, 1, 1, None, None, None, 2, None, None) == _cabi.LA_ERR_NULL_ARG
    for size in (0, 1, 3, 8, -4):
        assert bm(m, 0, 0, 1, 1, 1, 1, None, None, buf, size, None, None) == _cabi.LA_ERR_DTYPE, size
    for size in (2, 4):
        assert bm(m, 0, 0, 0, 1, 1, 1, None, None, buf, size, None, None) == _cabi.LA_ERR_SHAPE
        assert bm(m, 0, 0, 1, 1, 1, 0, None, None, buf, size, None, None) == _cabi.LA_ERR_SHAPE
        assert bm(m, 0, -4, 1, 1, 1, 1, None, None, buf, size, None, None) == _cabi.LA_ERR_STRIDE
    assert bm(m, 0, 0, 1, 1, 1, 32767, None, None, buf, 2, None, None) == _cabi.LA_ERR_SEQLEN
    assert bm(m, 0, 0, 1 << 20, 1 << 10, 1 << 10, 32767, None, None, buf, 4, None, None) == _cabi.LA_ERR_SHAPE


def test_object_keeps_int16_lists_and_rebuilds_on_a_dtype_change(rec):
    q = torch.zeros(1, 300, 2, 128, dtype=torch.bfloat16)
    a32, a16 = L.LiteAttention(max_batch_size=2), L.LiteAttention(max_batch_size=2, list_dtype=torch.int16)
    assert a32.list_dtype == torch.int32 and a16.list_dtype == torch.int16
    a32(q, q, q)
    a16(q, q, q)
    assert a16._skip_list.dtype == torch.int16 and a16._skip_list.nbytes * 2 == a32._skip_list.nbytes
    assert torch.equal(a16._skip_list.to(torch.int32), a32._skip_list)
    assert rec.calls[-1]["read"].dtype == rec.calls[-1]["write"].dtype == torch.int16
    assert rec.calls[-1]["must_do"].dtype == torch.int32                    # the must-do row stays int32
    assert a16._shape_key[-1] == torch.int16 and a32._shape_key[-1] == torch.int32
    assert a16.get_skip_fraction() == a32.get_skip_fraction() == 0.0
    q2 = torch.zeros(2, 300, 2, 128, dtype=torch.bfloat16)                  # growth keeps the element type
    a16(q2, q2, q2)
    assert a16._skip_list.dtype == torch.int16 and a16._skip_list.shape[1] == 2
    a16.preallocate(q, q, batch=2)
    assert a16._skip_list.dtype == torch.int16
    a16.list_dtype = torch.int32                                            # part of the re-init key
    a16(q, q, q)
    assert a16._skip_list.dtype == torch.int32 and a16._phase == 1
    sp = L.SeqParallelLiteAttention(2, list_dtype=torch.int16)
    assert all(x.list_dtype == torch.int16 for x in sp.lite_attention)
    sp(q, q, q, split_idx=1)
    assert sp.lite_attention[1]._skip_list.dtype == torch.int16


def test_state_dict_roundtrip_int32_int16_int32(rec):
    q = torch.zeros(1, 300, 2, 128, dtype=torch.bfloat16)
    a32 = L.LiteAttention(threshold=-4.0, max_batch_size=1)
    a32(q, q, q)
    a32._skip_list[1, 0, 0, 0, :5] = torch.tensor([4, 4, 3, 1, 0], dtype=torch.int32)
    st32 = a32.state_dict()
    assert st32["list_dtype"] == "int32" and st32["skip_list"].dtype == torch.int32
    a16 = L.LiteAttention(list_dtype=torch.int16)
    a16.load_state_dict(st32)
    assert a16._skip_list.dtype == torch.int16 and a16._phase == 1 and a16.threshold == -4.0
    assert torch.equal(a16._skip_list.to(torch.int32), a32._skip_list)
    a16(q, q, q)                                                            # same shapes: no re-init, continues the ping-pong
    assert a16._phase == 0 and rec.calls[-1]["read"].dtype == torch.int16 and rec.calls[-1]["read"][0, 0, 0, :5].tolist() == [4, 4, 3, 1, 0]
    st16 = a16.state_dict()
    assert st16["list_dtype"] == "int16" and st16["skip_list"].dtype == torch.int16
    back = L.LiteAttention()
    back.load_state_dict(st16)
    assert back._skip_list.dtype == torch.int32 and torch.equal(back._skip_list, a32._skip_list) and back._phase == 0
    legacy = {k: v for k, v in st32.items() if k != "list_dtype"}           # a checkpoint from before the key existed
    old = L.LiteAttention(list_dtype=torch.int16)
    old.load_state_dict(legacy)
    assert old._skip_list.dtype == torch.int16
    # narrowing a list that holds a value above 32 767 is refused, and nothing wraps
    bad = dict(st32, skip_list=st32["skip_list"].clone())
    bad["skip_list"][0, 0, 0, 0, 1] = 40000
    with pytest.raises(ValueError, match="int16"):
        L.LiteAttention(list_dtype=torch.int16).load_state_dict(bad)
    wide = L.LiteAttention()
    wide.load_state_dict(bad)                                               # int32 keeps it as it is
    assert int(wide._skip_list[0, 0, 0, 0, 1]) == 40000
    with pytest.raises(ValueError):
        sl.convert_lists(torch.tensor([-40000], dtype=torch.int32), torch.int16)


def test_host_blockmask_lists_take_a_dtype():
    mask = torch.rand(2, 5, 9) > 0.4
    mask[..., 0] = True
    from liteattention_amd import compat
    l32 = compat.blockmask_to_lists(mask)
    l16 = compat.blockmask_to_lists(mask, dtype=torch.int16)
    assert l32.dtype == torch.int32 and l16.dtype == torch.int16 and torch.equal(l16.to(torch.int32), l32)
    with pytest.raises(ValueError):
        compat.blockmask_to_lists(mask, dtype=torch.int64)


def test_env_sets_the_class_default():
    code = ("import sys; sys.path.insert(0, %r)\nimport torch\nimport liteattention_amd as L\nfrom liteattention_amd import _cabi\n"
            "assert _cabi.default_list_dtype() == torch.int16\n"
            "assert L.LiteAttention().list_dtype == torch.int16\n"
            "assert L.LiteAttention(list_dtype=torch.int32).list_dtype == torch.int32\n"
            "assert L.SeqParallelLiteAttention(2).lite_attention[0].list_dtype == torch.int16\n" % ROOT)
    assert subprocess.run([sys.executable, "-c", code], env=dict(os.environ, LA_LIST_DTYPE="int16")).returncode == 0
    bad = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, LA_LIST_DTYPE="int8"), capture_output=True, text=True)
    assert bad.returncode != 0 and "LA_LIST_DTYPE" in bad.stderr
    assert _cabi.default_list_dtype() == torch.int32 or os.environ.get("LA_LIST_DTYPE") == "int16"
