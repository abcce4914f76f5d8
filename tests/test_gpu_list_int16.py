"""GPU: int16 skip lists (LA_FLAG_LIST_INT16) against int32 ones, on every kernel that reads or writes lists.

The element type of a list cannot change arithmetic: the kernels expand a read-list row into the same LDS walk whatever it is read
from, and serialise the same votes into the write list. So the bar is BIT IDENTITY, no tolerance: every case runs the same inputs
twice from the same initial lists over consecutive calls (ping-pong, as ``LiteAttention`` does it) - once with int32 lists, once with
int16 - and at every step O and LSE are ``torch.equal`` and the int16 write list, widened, equals the int32 one over the WHOLE tensor
(entries behind a row's length included: both runs start from the same bytes, so what a writer leaves alone is equal too).

Inputs are the fragmenting generator of tests/helpers.py (a hot key tile every 3rd or 4th, slowly varying over steps) at thr = -3,
with a key range long enough that the lists of the later steps hold more than 64 ranges per row: the second pass of the wave-parallel
expander (``expand_read_list`` / ``expand_read_list_bits``) and the carry of the wave-parallel writers run on int16 rows too. Every
main case asserts that beforehand on the int32 run's step-3 read list.

One mid-size case goes against the tiled oracle (which speaks int32: the lists are widened first) under the tolerances the
fragmented-list tests use; a guard test puts the int16 lists inside a larger buffer of sentinel halfwords at an odd offset."""
import math

import pytest
import torch

from helpers import fragmented_qkv, structured_qkv

pytestmark = pytest.mark.gpu
F8 = torch.float8_e4m3fn
I16, I32 = torch.int16, torch.int32
MODES = {"default": {}, "half": {"LA_VOTE": "half"}, "v2": {"LA_FWD_KERNEL": "v2"}}
SQ, SK_ODD, SK_EVEN = 1100, 24000, 23900          # 375 (odd) / 374 (even) key tiles of 64; 5 q-tiles of 256 rows (9 of 128), the last ragged
STEPS, THR = 5, -3.0
SENTINEL = 0x5A5A


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for name in ("LA_VOTE", "LA_FWD_KERNEL", "LA_SCHED", "LA_LIST_DTYPE"):
        monkeypatch.delenv(name, raising=False)


def _mode(monkeypatch, mode, static=False):
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    if static:
        monkeypatch.setenv("LA_SCHED", "static")


def _cast(dtype):
    return {"bf16": lambda x: x.bfloat16(), "fp16": lambda x: x.half(), "fp8": lambda x: x.to(F8)}[dtype]


def _torch_dtype(dtype):
    return {"bf16": torch.bfloat16, "fp16": torch.float16, "fp8": F8}[dtype]


def _raw_inputs(B, Sq, Sk, H, D, step, Hk=None, seed=5):
    q, k, v = fragmented_qkv(B, Sq, H, D, seed=seed, step=step, steps=STEPS, dtype=torch.float32, Sk=Sk)
    if Hk is not None and Hk != H:                 # GQA: every (H / Hk)-th head of the generated K / V
        k, v = k[:, :, :: H // Hk].contiguous(), v[:, :, :: H // Hk].contiguous()
    return q, k, v


def _inputs(dtype, B, Sq, Sk, H, D, step, Hk=None, seed=5):
    return [_cast(dtype)(x).cuda() for x in _raw_inputs(B, Sq, Sk, H, D, step, Hk, seed)]


def _must_do(kind, B, H, Qt, Kt, bn, Sk):
    """(tensor or None, is_1d): absent / one range / three ranges (the serial writer) as ONE shared row, or the 4-D repeat."""
    from liteattention_amd import skip_lists as sl
    if kind == "absent":
        return None, False
    tokens = [Sk // 2, max(0, Sk // 2 - 1500)] if kind in ("1d_single", "4d") else [Sk - 200, Sk - 900, Sk // 2, Sk // 2 - 400, 300, 0]
    row = sl.must_do_row(tokens, bn, Kt + 1, "cuda")
    if kind == "4d":
        return row.repeat(B, H, Qt, 1).contiguous(), False
    return row, True


def _ranges(lst):
    return int(lst[..., 0].max()) // 2


def _pingpong(call, lists, B, steps=STEPS, frag_step=3, need_frag=True, tag=""):
    """`lists` = {I32: [2, ...] int32, I16: the same bytes narrowed}. Runs `call(step, read, write)` for both element types at every
    step and compares; returns the int32 lists and the last outputs."""
    assert torch.equal(lists[I16].to(I32), lists[I32])
    last = None
    for step in range(steps):
        rd, wr = step % 2, 1 - step % 2
        if need_frag and step == frag_step:
            n = _ranges(lists[I32][rd][:B])
            assert n > 64, f"{tag}: the step-{frag_step} read list holds at most {n} ranges per row: the second expander pass is not exercised"
        before = {t: lists[t][rd].clone() for t in (I32, I16)}
        o32, l32 = call(step, lists[I32][rd], lists[I32][wr])
        o16, l16 = call(step, lists[I16][rd], lists[I16][wr])
        torch.cuda.synchronize()
        assert torch.equal(o16, o32), f"{tag}: O differs at step {step}"
        assert torch.equal(l16, l32), f"{tag}: LSE differs at step {step}"
        assert lists[I16].dtype == I16 and torch.equal(lists[I16][wr].to(I32), lists[I32][wr]), f"{tag}: write list differs at step {step}"
        for t in (I32, I16):
            assert torch.equal(lists[t][rd], before[t]), f"{tag}: the read list was written at step {step}"
        last = (o32, l32)
    assert int(lists[I32][..., 0].min()) >= 0 and int(lists[I32][..., 1:].max()) < lists[I32].shape[-1] - 1
    return lists[I32], last


def _fixed_case(monkeypatch, mode, dtype, D, *, B=1, H=2, Hk=None, Sq=SQ, Sk=SK_ODD, must_do="absent", windows=None, static=False,
                need_frag=True, B_alloc=None):
    import liteattention_amd as L
    from liteattention_amd.flash_attn_interface import mha_fwd
    _mode(monkeypatch, mode, static)
    bm, bn = L.get_tile_sizes(D, 1 if dtype == "fp8" else 2)
    Qt, Kt = math.ceil(Sq / bm), math.ceil(Sk / bn)
    l32 = L.LiteAttention.init_skip_list(B_alloc or B, Sq, H, D, False, _torch_dtype(dtype), "cuda", seq_len_k=Sk)
    l16 = L.LiteAttention.init_skip_list(B_alloc or B, Sq, H, D, False, _torch_dtype(dtype), "cuda", seq_len_k=Sk, list_dtype=I16)
    assert tuple(l32.shape) == (2, B_alloc or B, H, Qt, Kt + 1) and l16.nbytes * 2 == l32.nbytes
    md, md_1d = _must_do(must_do, B_alloc or B, H, Qt, Kt, bn, Sk)
    win = None
    if windows == "two":                           # two windows that cover every q-tile (half vote: the first holds an even number)
        first = 2 if Qt < 6 else 4
        win = [(0, first), (first, Qt - first)]
    data = [_inputs(dtype, B, Sq, Sk, H, D, step, Hk) for step in range(STEPS)]

    def call(step, rd, wr):
        out, lse, *_ = mha_fwd(*data[step], attn_read_list=rd, attn_write_list=wr, attn_must_do_list=md, thr=THR,
                               _must_do_is_1d=md_1d, _q_windows=win)
        return out, lse
    tag = f"{mode}/{dtype}/D{D}/{must_do}"
    return _pingpong(call, {I32: l32, I16: l16}, B, need_frag=need_frag, tag=tag)


# ---- the grid ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("mode,D", [("default", 64), ("default", 96), ("default", 128), ("half", 64), ("half", 96), ("half", 128),
                                    ("v2", 64), ("v2", 128)])
def test_16bit_kernels_every_vote(monkeypatch, mode, D, dtype):
    _fixed_case(monkeypatch, mode, dtype, D, Sk=SK_ODD if D != 96 else SK_EVEN)


@pytest.mark.parametrize("D", [64, 96, 128, 192, 256])
def test_e4m3_every_head_dim(monkeypatch, D):
    _fixed_case(monkeypatch, "default", "fp8", D, Sk=SK_EVEN if D in (64, 192) else SK_ODD)


@pytest.mark.parametrize("must_do", ["1d_single", "1d_multi", "4d"])
@pytest.mark.parametrize("mode,dtype", [("default", "bf16"), ("half", "bf16"), ("v2", "fp16"), ("default", "fp8")])
def test_must_do_forms(monkeypatch, mode, dtype, must_do):
    _fixed_case(monkeypatch, mode, dtype, 128, Sk=SK_EVEN, must_do=must_do)


@pytest.mark.parametrize("mode,dtype,D", [("default", "bf16", 128), ("half", "fp16", 64), ("v2", "bf16", 128), ("default", "fp8", 96)])
def test_static_scheduling(monkeypatch, mode, dtype, D):
    """LA_FLAG_STATIC_SCHED: one workgroup per item, no prefetch of the next item's walk."""
    _fixed_case(monkeypatch, mode, dtype, D, static=True)


@pytest.mark.parametrize("mode,dtype,D", [("default", "bf16", 128), ("half", "bf16", 96), ("default", "fp8", 128)])
def test_two_q_tile_windows(monkeypatch, mode, dtype, D):
    _fixed_case(monkeypatch, mode, dtype, D, windows="two", must_do="1d_single")


@pytest.mark.parametrize("mode,dtype,D", [("default", "bf16", 128), ("half", "fp16", 128), ("v2", "bf16", 64), ("default", "fp8", 256)])
def test_batch_2_and_gqa(monkeypatch, mode, dtype, D):
    _fixed_case(monkeypatch, mode, dtype, D, B=2, H=4, Hk=2, Sq=700, must_do="1d_multi")


@pytest.mark.parametrize("Sk", [64, 100, 7 * 64, 8 * 64 - 3])
@pytest.mark.parametrize("mode,dtype,D", [("default", "bf16", 128), ("half", "bf16", 64), ("v2", "fp16", 128), ("default", "fp8", 128),
                                          ("default", "fp8", 192)])
def test_tiny_key_ranges(monkeypatch, mode, dtype, D, Sk):
    """k_tiles of 1, 2, 7 and 8: rows of 2, 3, 8 and 9 entries - the pair behind an odd row reads as (0, 0), a row of two entries holds
    a count and a start only. (Too short to fragment: the > 64 ranges assertion belongs to the cases above.)"""
    _fixed_case(monkeypatch, mode, dtype, D, B=2, H=2, Sq=600, Sk=Sk, must_do="absent" if Sk == 64 else "1d_single", need_frag=False)


@pytest.mark.parametrize("mode,dtype,D", [("default", "bf16", 128), ("half", "bf16", 128), ("default", "fp16", 64), ("default", "fp8", 128)])
def test_packed_batch_with_cu_seqlens(monkeypatch, mode, dtype, D):
    """Lists under cu_seqlens: the geometry of the maxima, row (b, h, m) over sequence b's own key tiles; one sequence is short in q and
    in k (its q-tiles past the end and its key tiles past its length are neither read nor written)."""
    import liteattention_amd as L
    from liteattention_amd.flash_attn_interface import mha_fwd
    _mode(monkeypatch, mode)
    H = 2
    sq, sk = [SQ, 390], [SK_ODD, 9000]
    bm, bn = L.get_tile_sizes(D, 1 if dtype == "fp8" else 2)
    l32 = L.LiteAttention.init_skip_list(2, max(sq), H, D, False, _torch_dtype(dtype), "cuda", seq_len_k=max(sk))
    # the short sequence starts from ITS full range (tile indices are relative to the sequence)
    l32[:, 1, :, :, 1] = math.ceil(sk[1] / bn) - 1
    l16 = l32.to(I16)
    cu_q = torch.tensor([0, sq[0], sum(sq)], dtype=torch.int32, device="cuda")
    cu_k = torch.tensor([0, sk[0], sum(sk)], dtype=torch.int32, device="cuda")
    data = []
    for step in range(STEPS):
        parts = [_raw_inputs(1, sq[b], sk[b], H, D, step, seed=5 + b) for b in range(2)]
        data.append([_cast(dtype)(torch.cat([p[i][0] for p in parts]).contiguous()).cuda() for i in range(3)])

    def call(step, rd, wr):
        out, lse, *_ = mha_fwd(*data[step], cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, max_seqlen_q=max(sq), max_seqlen_k=max(sk),
                               attn_read_list=rd, attn_write_list=wr, thr=THR)
        return out, lse
    _pingpong(call, {I32: l32, I16: l16}, 2, tag=f"varlen/{mode}/{dtype}/D{D}")


# ---- against the oracle ------------------------------------------------------------------------------------------------------
def test_mid_size_int16_lists_match_the_oracle():
    """S = 6 100 (96 key tiles), bf16 head_dim 128, 4 steps through ``LiteAttention(list_dtype=torch.int16)``: O, LSE and the write list
    against the tiled oracle walking the SAME (widened) read list, under the tolerances of the fragmented-list tests."""
    from test_gpu_fragmented import _setup
    from test_gpu_parity import _compare_lists
    L, orc, bm, bn, cast, p_round, tol, lse_tol = _setup("bf16", 128)
    B, S, H, thr, steps = 1, 6100, 4, -3.0, 4
    Qt, Kt = math.ceil(S / bm), math.ceil(S / bn)
    att = L.LiteAttention(threshold=thr, max_batch_size=B, list_dtype=I16)
    md_row = orc.expand_must_do_ref([0, 0], bn, Kt + 1)
    margins = torch.empty(B, H, Qt, Kt)
    max_len, borderline = 0, 0
    for step in range(steps):
        q, k, v = [cast(x) for x in fragmented_qkv(B, S, H, 128, seed=5, step=step, steps=steps, dtype=torch.float32)]
        rd_idx = att._phase if att._skip_list is not None else 0
        out, lse = att(q.cuda(), k.cuda(), v.cuda(), return_softmax_lse=True)
        assert att._skip_list.dtype == I16
        rd, wr = att._skip_list[rd_idx].cpu().to(I32), att._skip_list[1 - rd_idx].cpu().to(I32)
        max_len = max(max_len, int(rd[..., 0].max()))
        wr_orc = torch.zeros_like(wr)
        o_ref, lse_ref, n_tiles = orc.qkskip_fwd(q, k, v, block_m=bm, block_n=bn, read_list=rd, write_list=wr_orc,
                                                 must_do_list=md_row, thr=thr, margins=margins, p_round=p_round)
        assert n_tiles == orc.listed_tiles(rd[:B])
        assert (out.float().cpu() - o_ref).abs().max().item() <= tol(o_ref), f"step {step}"
        assert (lse.cpu() - lse_ref).abs().max().item() <= lse_tol, f"step {step}"
        bad, border = _compare_lists(orc, rd, wr, wr_orc, margins, thr, B)
        assert bad == 0, f"step {step}: {bad} rows differ from the oracle with no borderline tile"
        borderline += border
    assert max_len >= 20, f"longest read row holds {max_len // 2} ranges: the lists did not fragment"
    assert borderline <= 4


# ---- memory safety -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,dtype,D", [("default", "bf16", 128), ("half", "bf16", 128), ("v2", "fp16", 128), ("default", "fp8", 128),
                                          ("default", "fp16", 64)])
def test_sentinels_around_unaligned_int16_lists_stay_intact(monkeypatch, mode, dtype, D):
    """The int16 lists are a view into a larger int16 buffer filled with a sentinel halfword: in front of them, behind them and - with
    B_alloc = 3 for a batch of 2 - in the rows of the batch entry no launch touches. Kt + 1 is odd and the view starts at an odd element,
    so rows start at addresses that are 2-byte but not 4-byte aligned: a 32-bit access to such a row would fault or damage the neighbour.
    Three calls (both buffers get written); results equal the int32 run's, every sentinel survives."""
    import liteattention_amd as L
    from liteattention_amd.flash_attn_interface import mha_fwd
    _mode(monkeypatch, mode)
    B, B_alloc, H, Sq, Sk = 2, 3, 2, 700, SK_EVEN
    bm, bn = L.get_tile_sizes(D, 1 if dtype == "fp8" else 2)
    Qt, Kt = math.ceil(Sq / bm), math.ceil(Sk / bn)
    assert (Kt + 1) % 2 == 1
    l32 = L.LiteAttention.init_skip_list(B, Sq, H, D, False, _torch_dtype(dtype), "cuda", seq_len_k=Sk)
    n_used, n_alloc, front, back = B * H * Qt * (Kt + 1), B_alloc * H * Qt * (Kt + 1), 37, 1001
    bufs, views = [], []
    for i in range(2):
        buf = torch.full((front + n_alloc + back,), SENTINEL, dtype=I16, device="cuda")
        view = buf[front: front + n_alloc].view(B_alloc, H, Qt, Kt + 1)
        assert view.is_contiguous() and view.data_ptr() % 4 == 2 and (view.data_ptr() + 2 * (Kt + 1)) % 4 == 0
        view[:B] = l32[i].to(I16)
        bufs.append(buf)
        views.append(view)
    md, md_1d = _must_do("1d_single", B, H, Qt, Kt, bn, Sk)
    for step in range(3):
        q, k, v = _inputs(dtype, B, Sq, Sk, H, D, step)
        rd, wr = step % 2, 1 - step % 2
        o32, s32, *_ = mha_fwd(q, k, v, attn_read_list=l32[rd], attn_write_list=l32[wr], attn_must_do_list=md, thr=THR, _must_do_is_1d=md_1d)
        o16, s16, *_ = mha_fwd(q, k, v, attn_read_list=views[rd], attn_write_list=views[wr], attn_must_do_list=md, thr=THR, _must_do_is_1d=md_1d)
        torch.cuda.synchronize()
        assert torch.equal(o16, o32) and torch.equal(s16, s32), step
        assert torch.equal(views[wr][:B].to(I32), l32[wr]), step
        for buf in bufs:
            assert bool((buf[:front] == SENTINEL).all()), f"step {step}: a halfword in front of the lists was written"
            assert bool((buf[front + n_used:] == SENTINEL).all()), f"step {step}: a halfword behind the batch's rows was written"
    assert _ranges(l32[1]) > 8                                           # and the lists did fragment


# ---- the two _ex entry points ------------------------------------------------------------------------------------------------
def test_blockmask_to_lists_int16_equals_int32():
    import ctypes
    from liteattention_amd import _cabi, compat
    g = torch.Generator().manual_seed(3)
    for shape in ((2, 3, 5, 301), (1, 2, 4, 6), (2, 1, 3, 1), (1, 1, 2, 5000)):       # 5000 tiles: the un-staged kernel (LDS stage > 64 KiB)
        mask = (torch.rand(*shape, generator=g) > 0.45).cuda()
        mask[..., 0, :] = False                                          # rows that keep nothing: counted in empty_rows
        n_empty = int((~mask.any(-1)).sum())
        B, H, Qt, Kt = shape
        got = {}
        for dt in (I32, I16):
            lists = torch.full((B, H, Qt, Kt + 1), -7, dtype=dt, device="cuda")
            empty = torch.full((1,), -1, dtype=torch.int32, device="cuda")
            m8 = mask.view(torch.uint8)
            rc = _cabi.load().la_blockmask_to_lists_ex(m8.data_ptr(), m8.stride(0), m8.stride(1), B, H, Qt, Kt, None, None, lists.data_ptr(),
                                                       lists.element_size(), empty.data_ptr(), torch.cuda.current_stream().cuda_stream)
            assert rc == _cabi.LA_OK
            torch.cuda.synchronize()
            got[dt] = (lists, int(empty.item()))
        assert torch.equal(got[I16][0].to(I32), got[I32][0]) and got[I16][1] == got[I32][1] == n_empty >= B * H
        old = torch.empty((B, H, Qt, Kt + 1), dtype=I32, device="cuda")
        rc = _cabi.load().la_blockmask_to_lists(m8.data_ptr(), m8.stride(0), m8.stride(1), B, H, Qt, Kt, None, None, old.data_ptr(), None,
                                                torch.cuda.current_stream().cuda_stream)
        assert rc == _cabi.LA_OK and torch.equal(old, got[I32][0])
        mask[..., 0] = True                                              # every row keeps tile 0: representable, with k_tiles_valid too
        kv = torch.tensor([max(1, Kt // 2)] * B)
        a = compat.blockmask_to_lists(mask, k_tiles_valid=kv, batch=B, heads=H)
        b = compat.blockmask_to_lists(mask, k_tiles_valid=kv, batch=B, heads=H, dtype=I16)
        assert a.dtype == I32 and b.dtype == I16 and torch.equal(b.to(I32), a)
        assert torch.equal(compat.blockmask_to_lists(mask.cpu(), dtype=I16).cuda(), compat.blockmask_to_lists(mask, dtype=I16))
    assert ctypes.sizeof(ctypes.c_int16) == 2


def test_skip_list_stats_counts_the_same_on_both_element_types(monkeypatch):
    import liteattention_amd as L
    from liteattention_amd import _cabi
    from oracle import oracle as orc
    l32, _ = _fixed_case(monkeypatch, "default", "bf16", 128, B=2, H=2, Sq=700, Sk=SK_EVEN)
    for lst in (l32[0], l32[1]):
        c32, c16 = L.skip_list_stats(lst), L.skip_list_stats(lst.to(I16))
        assert torch.equal(c32, c16) and int(c32[0]) == orc.listed_tiles(lst.cpu()) and int(c32[1]) == lst.shape[0] * lst.shape[1] * lst.shape[2]
        assert torch.equal(L.skip_list_stats(lst.to(I16), batch=1), L.skip_list_stats(lst, batch=1))
        assert L.LiteAttention.calc_percentage(lst.to(I16)) == L.LiteAttention.calc_percentage(lst) < 0.9
        out = torch.empty(2, dtype=torch.int64, device="cuda")
        rc = _cabi.load().la_skip_list_stats(lst.data_ptr(), lst.shape[0], lst.shape[1], lst.shape[2], lst.shape[3] - 1, out.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream)
        assert rc == _cabi.LA_OK and torch.equal(out, c32)               # the int32 entry point is the element-size-4 case


# ---- the object and a captured graph -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_object_with_int16_lists_over_6_steps(dtype):
    import liteattention_amd as L
    B, H, D = 2, 2, 128
    a32 = L.LiteAttention(threshold=THR, max_batch_size=B)
    a16 = L.LiteAttention(threshold=THR, max_batch_size=B, list_dtype=I16)
    for step in range(6):
        q, k, v = _inputs(dtype, B, 700, SK_EVEN, H, D, step)
        o32, s32 = a32(q, k, v, return_softmax_lse=True, must_do_list=[9000, 8000])
        o16, s16 = a16(q, k, v, return_softmax_lse=True, must_do_list=[9000, 8000])
        assert torch.equal(o16, o32) and torch.equal(s16, s32), step
        assert a16.get_skip_fraction() == a32.get_skip_fraction(), step
    assert a16._skip_list.dtype == I16 and a16._skip_list.nbytes * 2 == a32._skip_list.nbytes
    assert torch.equal(a16._skip_list.to(I32), a32._skip_list)
    assert a16.get_skip_fraction() > 0.2 and _ranges(a32.current_read_list()) > 64
    # a checkpoint of one element type continues in the other
    st = a16.state_dict()
    cont = L.LiteAttention(list_dtype=I32)
    cont.load_state_dict(st)
    q, k, v = _inputs(dtype, B, 700, SK_EVEN, H, D, 5)
    assert torch.equal(cont(q, k, v), a32(q, k, v)) and torch.equal(cont._skip_list, a32._skip_list)


def test_hip_graph_replay_of_int16_calls_equals_eager():
    """Modelled on tests/test_gpu_graph.py: two consecutive calls (phases 0 and 1) per graph, replayed on new inputs."""
    import liteattention_amd as L
    B, S, H, D, steps = 1, 2304, 4, 128, 8
    data = [[x.cuda() for x in structured_qkv(B, S, H, D, seed=400, alpha=9.0 - 0.3 * t)] for t in range(steps)]
    att_32 = L.LiteAttention(threshold=THR, max_batch_size=B)
    att_e = L.LiteAttention(threshold=THR, max_batch_size=B, list_dtype=I16)
    outs_e = [att_e(*data[t], return_softmax_lse=True) for t in range(steps)]
    for t in range(steps):
        o, lse = att_32(*data[t], return_softmax_lse=True)
        assert torch.equal(o, outs_e[t][0]) and torch.equal(lse, outs_e[t][1])
    att_g = L.LiteAttention(threshold=THR, max_batch_size=B, list_dtype=I16)
    for t in (0, 1):
        o, lse = att_g(*data[t], return_softmax_lse=True)
        assert torch.equal(o, outs_e[t][0])
    static = [[torch.empty_like(x) for x in data[0]] for _ in range(2)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o0, l0 = att_g(*static[0], return_softmax_lse=True)
        o1, l1 = att_g(*static[1], return_softmax_lse=True)
    for t in range(2, steps, 2):
        for i in range(2):
            for buf, src in zip(static[i], data[t + i]):
                buf.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o0, outs_e[t][0]) and torch.equal(l0, outs_e[t][1]), t
        assert torch.equal(o1, outs_e[t + 1][0]) and torch.equal(l1, outs_e[t + 1][1]), t + 1
    assert att_g._skip_list.dtype == I16 and torch.equal(att_g._skip_list, att_e._skip_list)
    assert torch.equal(att_g._skip_list.to(I32), att_32._skip_list)
    assert att_g.get_skip_fraction() == att_e.get_skip_fraction() > 0.05
