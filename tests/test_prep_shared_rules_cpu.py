"""CPU: the rules la_qk_prep, la_qk_prep_fp8 and la_qk_prep_smooth share, asked of all three with ONE list of violations: every entry
point answers a violation with the same code, and the code is the one the per-entry tests (test_qk_prep_cpu.py, test_qk_prep_fp8_cpu.py,
test_qk_prep_smooth_cpu.py) state for that rule. Every check answers before any HIP call, so no device is needed."""
import ctypes

import pytest

from liteattention_amd import _cabi

ENTRIES = {"la_qk_prep": _cabi.LaQkPrepArgs, "la_qk_prep_fp8": _cabi.LaQkPrepFp8Args, "la_qk_prep_smooth": _cabi.LaQkPrepSmoothArgs}
E4M3_ENTRIES = ("la_qk_prep_fp8", "la_qk_prep_smooth")
S, B = 60, 2                      # 60 rows: every position of the (3, 4, 5) grid


def _valid_args(entry, H=4, D=128):
    """Arguments of `entry` that pass every check, everything asked for (token norm, grid (3, 4, 5), the axes rotate all D / 2 pairs, one
    scale and one dot vector per head); no pointer is dereferenced on the host."""
    a = ENTRIES[entry]()
    a.struct_size = ctypes.sizeof(ENTRIES[entry])
    a.in_dtype, a.norm_mode = _cabi.LA_DTYPE_BF16, _cabi.LA_NORM_TOKEN
    a.x, a.out, a.weight = 0x10000, 0x20010, 0x30000
    a.x_batch_stride = a.out_batch_stride = S * H * D
    a.x_row_stride = a.out_row_stride = H * D
    a.x_head_stride = a.out_head_stride = D
    a.batch, a.seqlen, a.num_heads, a.head_dim = B, S, H, D
    a.eps, a.pos_offset = 1e-6, 0
    pairs = (D // 2 - 2 * (D // 6), D // 6, D // 6)
    for i, (e, n) in enumerate(zip((3, 4, 5), pairs)):
        a.rope_table[i], a.axis_extent[i], a.axis_pairs[i] = 0x40000 + 0x1000 * i, e, n
    if entry == "la_qk_prep":
        a.out_dtype = _cabi.LA_DTYPE_BF16
    else:
        a.heads_per_scale = 1
        a.descale, a.amax = 0x50004, 0x60004
        a.descale_batch_stride = a.amax_batch_stride = H
        a.descale_head_stride = a.amax_head_stride = 1
    if entry == "la_qk_prep_smooth":
        a.heads_per_dot = 1
        a.shift, a.colsum_part, a.dot_vec, a.dot_out = 0x70000, 0x80010, 0x90000, 0xa0004
        a.shift_batch_stride = a.dot_vec_batch_stride = H * D
        a.shift_head_stride = a.dot_vec_head_stride = D
    return a


def _rc(entry, a):
    return getattr(_cabi.load(), entry)(ctypes.byref(a), None)


def _set(**fields):
    def change(a):
        for k, v in fields.items():
            setattr(a, k, v)
    return change


def _item(array, i, v):
    def change(a):
        getattr(a, array)[i] = v
    return change


# (what is wrong, the shape (H, D) of the valid arguments it is applied to, the change, the code)
SHARED = [
    ("norm mode 3", (4, 128), _set(norm_mode=3), _cabi.LA_ERR_UNSUPPORTED),
    ("norm mode -1", (4, 128), _set(norm_mode=-1), _cabi.LA_ERR_UNSUPPORTED),
    ("batch 0", (4, 128), _set(batch=0), _cabi.LA_ERR_SHAPE),
    ("seqlen -1", (4, 128), _set(seqlen=-1), _cabi.LA_ERR_SHAPE),
    ("num_heads 0", (4, 128), _set(num_heads=0), _cabi.LA_ERR_SHAPE),
    ("head_dim 0", (4, 128), _set(head_dim=0), _cabi.LA_ERR_SHAPE),
    ("head_dim 12", (4, 128), _set(head_dim=12), _cabi.LA_ERR_HEAD_DIM),
    ("head_dim 264", (4, 128), _set(head_dim=264), _cabi.LA_ERR_HEAD_DIM),
    ("token norm over 65 * 256 elements", (65, 256), _set(), _cabi.LA_ERR_UNSUPPORTED),
    ("token norm over 2049 * 8 elements", (2049, 8), _set(), _cabi.LA_ERR_UNSUPPORTED),
    ("negative x row stride", (4, 128), _set(x_row_stride=-512), _cabi.LA_ERR_STRIDE),
    ("negative x batch stride", (4, 128), _set(x_batch_stride=-1), _cabi.LA_ERR_STRIDE),
    ("negative x head stride", (4, 128), _set(x_head_stride=-128), _cabi.LA_ERR_STRIDE),
    ("x row stride off 16 bytes", (4, 128), _set(x_row_stride=512 + 4), _cabi.LA_ERR_STRIDE),
    ("x head stride off 16 bytes", (4, 128), _set(x_head_stride=128 + 4), _cabi.LA_ERR_STRIDE),
    ("x batch stride off 16 bytes", (4, 128), _set(x_batch_stride=S * 512 + 2), _cabi.LA_ERR_STRIDE),
    ("x off 16 bytes", (4, 128), _set(x=0x10008), _cabi.LA_ERR_STRIDE),
    ("weight off 16 bytes", (4, 128), _set(weight=0x30004), _cabi.LA_ERR_STRIDE),
    ("table off 8 bytes", (4, 128), _item("rope_table", 1, 0x41004), _cabi.LA_ERR_STRIDE),
    ("negative axis pairs", (4, 128), _item("axis_pairs", 1, -1), _cabi.LA_ERR_SHAPE),
    ("more pairs than a head has", (4, 128), _item("axis_pairs", 2, 22), _cabi.LA_ERR_SHAPE),
    ("negative pos_offset", (4, 128), _set(pos_offset=-1), _cabi.LA_ERR_SHAPE),
    ("a rotated axis without a table", (4, 128), _item("rope_table", 1, None), _cabi.LA_ERR_NULL_ARG),
    ("axis extent 0", (4, 128), _item("axis_extent", 1, 0), _cabi.LA_ERR_SHAPE),
    ("pos_offset + seqlen past the grid", (4, 128), _set(pos_offset=1), _cabi.LA_ERR_SHAPE),
]
E4M3 = [
    ("heads_per_scale 0", (4, 128), _set(heads_per_scale=0), _cabi.LA_ERR_SHAPE),
    ("heads_per_scale 3 of 4 heads", (4, 128), _set(heads_per_scale=3), _cabi.LA_ERR_SHAPE),
    ("negative descale batch stride", (4, 128), _set(descale_batch_stride=-1), _cabi.LA_ERR_STRIDE),
    ("negative amax head stride", (4, 128), _set(amax_head_stride=-1), _cabi.LA_ERR_STRIDE),
    ("descale off by 2 bytes", (4, 128), _set(descale=0x50006), _cabi.LA_ERR_STRIDE),
    ("amax off by 2 bytes", (4, 128), _set(amax=0x60006), _cabi.LA_ERR_STRIDE),
    # more heads than a workgroup keeps scales for; head norm, or the token limit would answer first
    ("1025 heads", (1025, 8), _set(norm_mode=_cabi.LA_NORM_HEAD), _cabi.LA_ERR_UNSUPPORTED),
]


def _answers(entries, shape, change):
    got = {}
    for entry in entries:
        a = _valid_args(entry, *shape)
        change(a)
        got[entry] = _rc(entry, a)
    return got


@pytest.mark.parametrize("what,shape,change,code", SHARED, ids=[v[0] for v in SHARED])
def test_every_entry_point_answers_a_shared_rule_alike(what, shape, change, code):
    assert _answers(ENTRIES, shape, change) == dict.fromkeys(ENTRIES, code)


@pytest.mark.parametrize("what,shape,change,code", E4M3, ids=[v[0] for v in E4M3])
def test_both_e4m3_entry_points_answer_a_scale_rule_alike(what, shape, change, code):
    assert _answers(E4M3_ENTRIES, shape, change) == dict.fromkeys(E4M3_ENTRIES, code)


def test_the_arguments_the_violations_start_from_reach_the_last_check():
    """With the complaint planted in the LAST shared check alone, that is the code: nothing else is wrong with the arguments the lists
    start from, nor with the largest shapes inside the limits the lists step over (16384 elements under token norm, 1024 heads)."""
    planted = dict.fromkeys(ENTRIES, _cabi.LA_ERR_SHAPE)
    assert _answers(ENTRIES, (4, 128), _set(pos_offset=1)) == planted
    assert _answers(ENTRIES, (64, 256), _set(pos_offset=1)) == planted
    assert _answers(ENTRIES, (2048, 8), _set(pos_offset=1)) == planted
    assert _answers(ENTRIES, (1024, 8), _set(pos_offset=1, norm_mode=_cabi.LA_NORM_HEAD)) == planted


# ---- the Meta kernels of the two e4m3 ops --------------------------------------------------------------------------------------------------
META_CALLS = [
    ("qk_prep_fp8", dict(heads_per_scale=2)),
    ("qk_prep_fp8", dict(norm="head")),
    ("qk_prep_fp8", dict(amax_out="amax")),
    ("qk_prep_fp8", dict(descale="amax", pos_offset=3)),
    ("qk_prep_smooth", dict(heads_per_scale=2)),
    ("qk_prep_smooth", dict(norm=None, shift="vec")),
    ("qk_prep_smooth", dict(amax_out="amax", heads_per_dot=2)),
    ("qk_prep_smooth", dict(dot_vec="vec", dot_out="dots")),
    ("qk_prep_smooth", dict(colsum_part="part")),
]


@pytest.mark.parametrize("op,kwargs", META_CALLS, ids=[f"{op}-{'-'.join(kw)}" for op, kw in META_CALLS])
def test_the_e4m3_meta_kernels_return_out_whatever_else_is_given(op, kwargs):
    """The dispatcher drops trailing arguments that equal their schema defaults before it calls a Python kernel, so with out=None the
    last argument a kernel sees is whichever non-default one comes last: the result is still a new e4m3 tensor of x's shape, and `out`
    itself when it is given."""
    import torch
    import liteattention_amd  # noqa: F401  (registers the ops)
    f32 = dict(dtype=torch.float32, device="meta")
    x = torch.empty(2, 60, 4, 128, dtype=torch.bfloat16, device="meta")
    given = {"amax": torch.empty(2, 4, **f32), "vec": torch.empty(2, 4, 128, **f32), "dots": torch.empty(2, 4, 60, **f32),
             "part": torch.empty(4, 2, 4, 128, **f32)}
    kwargs = {k: given.get(v, v) if isinstance(v, str) and k != "norm" else v for k, v in kwargs.items()}
    fn = getattr(torch.ops.lite_attention, op)
    got = fn(x, **kwargs)
    assert got.shape == x.shape and got.dtype == torch.float8_e4m3fn and got.device.type == "meta"
    out = torch.empty(2, 60, 4, 128, dtype=torch.float8_e4m3fn, device="meta")
    assert fn(x, out=out, **kwargs) is out
