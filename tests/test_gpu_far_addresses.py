"""GPU: every forward body with operands more than 4 GiB from their base pointers (tests/far_cases.py; the layouts are proved wrap-safe by
tests/test_far_cases_cpu.py: a body that builds an offset in 32 bits gives wrong numbers here, it does not fault).

One module-scoped allocation of 14.4 GB, filled with byte 0xFF (NaN in bf16, fp16 and e4m3: poison and canary at once), holds q, k, v and
`out` of every case as strided views. Four axes carry the distance - the batch stride (2^33 bytes), the head stride (2^33 bytes), the row
stride (2^26 bytes, EXACTLY the largest K / V row stride la_fwd accepts: this is the accepting side of
tests/test_cabi.py::test_kv_row_stride_above_the_bound_is_refused) and the ``cu_seqlens`` row offset of a packed batch at that pitch.
Sq = Sk = 150 (three key tiles, the last one ragged).

Every case runs one problem twice - *clean* (contiguous tensors) and *far* (the views) - and asserts, with no tolerance of its own, what
tests/test_gpu_layout_poison.py asserts:

* `out`, `lse` and the write list BIT-IDENTICAL between the two runs;
* the clean run inside the body's existing oracle rule (``_check_against_oracle`` of tests/test_gpu_layout_poison.py);
* the q / k / v elements in the allocation unchanged;
* every byte of the allocation outside `out`'s elements still 0xFF (the views are refilled with 0xFF after the comparisons and the WHOLE
  allocation is scanned, in chunks of 1 GiB).

Bodies: the 23 of tests/test_gpu_layout_poison.py (dense on every axis; with lists on every axis where la_fwd serves them: a packed batch
with lists runs on the hand-scheduled bodies at head_dim <= 128 and on e4m3) and the half-vote bodies of head dims 64 / 96 / 128 (lists
only: a dense launch under LA_VOTE=half is the plain body). Lists (a row of Kt + 1 = 4 entries holds one range): the first q-tile lists
key tiles 2 and 1 and skips tile 0, the second 128-row q-tile lists 1 and 0 and skips the ragged tile 2; thr = -inf, a write list is given;
a packed batch lists every tile of each sequence but tile 0 of the first.

The last test is the e4m3 V^T workspace past 4 GiB: B = 16, H = Hk = 8, Sk = 262 208 (4 097 key tiles), head_dim 128, 4.296 GB of
prepared tiles in ONE launch (4 097 tiles fit one e4m3 walk; la_fwd's split of long dense walks starts later).

Measured on one MI355X, the module in a process of its own: 188 cases in 7.5 s of wall time - 187 far cases of about 10 ms each (two
launches, the oracle on 150 x 150 scores, a scan of 14.4 GB) and 3.5 s for the V^T test (8.6 GB of random e4m3 K / V, three oracle slices
of 262 208 keys; its errors: |O - oracle| 2.9e-3 .. 3.2e-3 under a tolerance of 5e-2, |LSE - oracle| 6e-6). Every body passed unchanged."""
import pytest
import torch

import far_cases as fc
import layout_cases as lc
import test_gpu_fp8 as f8
from far_cases import F8
from helpers import fp8_lse_tol, fp8_p_round
from test_gpu_half_vote import half          # noqa: F401  (fixture: LA_VOTE=half)
from test_gpu_layout_poison import BODIES, BF, NEG_INF, _bits_equal, _check_against_oracle, _descales, _dev, _ids, _setenv

pytestmark = pytest.mark.gpu
HALF_BODIES = [(f"half-bf16-d{D}", BF, D, {}) for D in (64, 96, 128)]
ROWS_Q0, ROWS_Q1 = [2, 1], [1, 0]                        # a row of Kt + 1 = 4 entries holds one range: q-tile 0 key tiles 2 1, q-tile 1 tiles 1 0
_STATE = {"dirty": True}


@pytest.fixture(scope="module")
def far_buf():
    """The one allocation. If it cannot be had the tests fail: they do not skip."""
    buf = torch.empty(fc.MAX_BYTES, dtype=torch.uint8, device="cuda")
    yield buf
    del buf
    torch.cuda.empty_cache()


@pytest.fixture()
def clean_buf(far_buf):
    """The allocation, every byte 0xFF on entry (refilled after a case that failed half-way)."""
    if _STATE["dirty"]:
        far_buf.fill_(fc.FILL)
    _STATE["dirty"] = True
    return far_buf


def _takes_packed_lists(body):
    _, dtype, D, env = body
    return dtype == F8 or (D <= 128 and "LA_FWD_KERNEL" not in env)


def _lists(case, body):
    """The read list, int32 on the CPU. Fixed-length: [B, H, Qt, 4]; packed: [3, H, 1, 3], the geometry of the maxima (70 rows)."""
    import liteattention_amd as L
    bm, bn = L.get_tile_sizes(body[2], 1 if body[1] == F8 else 2)
    assert bn == 64
    if not case.packed:
        Qt = -(-case.Sq // bm)
        return lc.list_rows([ROWS_Q0, ROWS_Q1][:Qt], case.B, case.H, k_tiles=3)
    assert max(fc.PACKED_LENS) <= min(bm, 2 * bn)
    rd = torch.zeros(len(fc.PACKED_LENS), case.H, 1, 3, dtype=torch.int32)
    rd[0, :, 0] = torch.tensor([2, 1, 1], dtype=torch.int32)             # 70 keys: tile 1 (6 keys) only
    rd[1:, :, 0] = torch.tensor([2, 0, 0], dtype=torch.int32)            # 60 / 20 keys: their one tile
    return rd


def _launch(case, ds, rd, cu):
    from liteattention_amd.flash_attn_interface import mha_fwd

    def launch(q, k, v, out):
        kw = dict(ds)
        wr = None
        if rd is not None:
            wr = torch.full_like(rd, -7)
            kw.update(attn_read_list=rd, attn_write_list=wr, thr=NEG_INF)
        if case.packed:
            kw.update(cu_seqlens_q=cu, cu_seqlens_k=cu, max_seqlen_q=max(fc.PACKED_LENS), max_seqlen_k=max(fc.PACKED_LENS))
        o, lse, *_ = mha_fwd(q, k, v, out=out, **kw)
        return o, lse, wr
    return launch


def _oracle(case, body, o, lse, wr, x, ds, rd):
    """The clean run under the body's existing rule; a packed batch per sequence (tests/test_gpu_layout_poison.py ``_varlen_clean``)."""
    if not case.packed:
        _check_against_oracle(body, o, lse, x["q"], x["k"], x["v"], ds, lists=None if rd is None else (rd, wr, None), ulps=0.75 if rd is None else 1.0)
        return
    cu = case.cu_seqlens().tolist()
    for b in range(len(fc.PACKED_LENS)):
        s = slice(cu[b], cu[b + 1])
        kt = -(-fc.PACKED_LENS[b] // 64)                       # the row of a sequence is its own Kt + 1 entries (tests/test_gpu_varlen_lists.py)
        lists = None if rd is None else (rd[b:b + 1, :, :, :kt + 1].contiguous(), wr[b:b + 1, :, :, :kt + 1].contiguous(), None)
        _check_against_oracle(body, o[s][None], lse[:, s][None], x["q"][s][None], x["k"][s][None], x["v"][s][None],
                              {n: t[b:b + 1] for n, t in ds.items()}, lists=lists, ulps=0.75 if rd is None else 1.0)


def _far_case(buf, body, axis, with_lists):
    _, dtype, D, _ = body
    case = fc.FarCase(axis, dtype, D)
    x = fc.inputs(case, seed=1000 * fc.AXES.index(axis) + D + (7 if with_lists else 0))
    g = torch.Generator().manual_seed(D + 3)
    nb = len(fc.PACKED_LENS) if case.packed else case.B
    ds = _descales(dtype, nb, case.Hk, g)
    rd = _lists(case, body) if with_lists else None
    xd, dsd = {n: t.cuda() for n, t in x.items()}, _dev(ds)
    rd_d = None if rd is None else rd.cuda()
    cu_d = case.cu_seqlens().cuda() if case.packed else None
    launch = _launch(case, dsd, rd_d, cu_d)

    # ---- clean: contiguous tensors, against the oracle
    o_c, lse_c, wr_c = launch(xd["q"], xd["k"], xd["v"], None)
    assert o_c.is_contiguous()
    _oracle(case, body, o_c.cpu(), lse_c.cpu(), None if wr_c is None else wr_c.cpu().to(torch.int32), x, ds, rd)

    # ---- far: the same problem on the views
    views = case.views(buf)
    for n in ("q", "k", "v"):
        assert lc.strides_ok(views[n], dtype == F8)
        lc.raw(views[n]).copy_(lc.raw(xd[n]))
    assert lc.strides_ok(views["out"], False)
    o_f, lse_f, wr_f = launch(views["q"], views["k"], views["v"], views["out"])
    torch.cuda.synchronize()
    assert o_f.data_ptr() == views["out"].data_ptr() and o_f.stride() == views["out"].stride()
    assert o_f.data_ptr() - buf.data_ptr() >= fc.ORIGIN
    assert _bits_equal(views["out"], o_c), "out differs"
    assert _bits_equal(lse_f, lse_c), "lse differs"
    assert (wr_f is None) == (wr_c is None) and (wr_f is None or torch.equal(wr_f, wr_c)), "write list differs"
    for n in ("q", "k", "v"):
        assert _bits_equal(views[n], xd[n]), f"{n} changed"
    # ---- nothing else written: with the four views refilled, the whole allocation is 0xFF again
    for vw in views.values():
        r = lc.raw(vw)
        r.fill_(fc.FILL if r.dtype == torch.uint8 else -1)
    assert fc.all_fill(buf), "a byte outside the four views changed"
    _STATE["dirty"] = False


@pytest.mark.parametrize("axis", fc.AXES)
@pytest.mark.parametrize("body", BODIES, ids=_ids(BODIES))
def test_dense_far_equals_clean(monkeypatch, clean_buf, body, axis):
    _setenv(monkeypatch, body)
    _far_case(clean_buf, body, axis, False)


LIST_CASES = [(b, ax) for b in BODIES for ax in fc.AXES if ax != "packed" or _takes_packed_lists(b)]


@pytest.mark.parametrize("body,axis", LIST_CASES, ids=[f"{b[0]}-{ax}" for b, ax in LIST_CASES])
def test_list_launch_far_equals_clean(monkeypatch, clean_buf, body, axis):
    _setenv(monkeypatch, body)
    _far_case(clean_buf, body, axis, True)


@pytest.mark.parametrize("axis", fc.AXES)
@pytest.mark.parametrize("body", HALF_BODIES, ids=_ids(HALF_BODIES))
def test_half_vote_far_equals_clean(half, clean_buf, body, axis):
    """LA_VOTE=half: 128-row list rows, two per workgroup item, which list different tiles here (fixed-length axes)."""
    import liteattention_amd as L
    assert L.get_tile_sizes(body[2], 2) == (128, 64)
    _far_case(clean_buf, body, axis, True)


def test_the_scan_sees_one_byte(clean_buf):
    """The canary check is not vacuous: one changed byte in the last chunk, and one in front of the first view, are seen."""
    for pos in (fc.MAX_BYTES - 3, fc.ORIGIN - 1, 0):
        clean_buf[pos] = 0xFE
        assert not fc.all_fill(clean_buf)
        clean_buf[pos] = fc.FILL
    assert fc.all_fill(clean_buf)
    _STATE["dirty"] = False


# --------------------------------------------------------------------------------------------- the e4m3 V^T workspace past 4 GiB
VT_B, VT_H, VT_SQ, VT_KT, VT_D = 16, 8, 64, 4097, 128
VT_SK = VT_KT * 64
VT_SHIFT = 16.0


def test_fp8_prepared_tiles_past_4gib(monkeypatch):
    """e4m3 head_dim 128, dense: the prepared V^T tiles [B, Hk, Kt] of 8 KiB take 16 * 8 * 4 097 * 8 192 = 4.296 GB, so the tiles 3 969 ..
    4 096 of the last (batch, head) lie past 2^32 bytes in the workspace - the last slice is also the first whose tile offset
    (b * Hk + hk) * Kt * 8192 crosses 2^32. V of exactly those key rows (254 016 ..) is shifted by +16 in every (batch, head): with
    near-uniform attention over 262 208 random keys O would otherwise be ~0.003, inside the absolute term of the fp8 tolerance whatever
    V was read; with the shift every output is about 16 * 128 / 4 097 = 0.5, and a prepare pass or a body that wraps the tile offset to
    the front of the workspace (unshifted tiles, or tiles never written) misses it by that much. Three (b, h) slices are held to the C
    oracle under the tolerances of tests/test_gpu_fp8.py: the first, a middle one and the last; all of out and lse must be finite."""
    import ctypes

    from liteattention_amd import _cabi
    from liteattention_amd.flash_attn_interface import mha_fwd
    from oracle import oracle as orc
    for name in ("LA_FWD_KERNEL", "LA_FP8_P", "LA_VOTE"):
        monkeypatch.delenv(name, raising=False)
    a = _cabi.LaFwdArgs()
    a.struct_size, a.dtype = ctypes.sizeof(_cabi.LaFwdArgs), _cabi.LA_DTYPE_FP8_E4M3
    a.batch, a.seqlen_q, a.seqlen_k, a.num_heads, a.num_heads_k, a.head_dim, a.head_dim_v = VT_B, VT_SQ, VT_SK, VT_H, VT_H, VT_D, VT_D
    tiles_bytes = VT_B * VT_H * VT_KT * 8192
    assert tiles_bytes > 1 << 32 and _cabi.load().la_fwd_workspace_bytes(ctypes.byref(a)) == tiles_bytes + 1024      # one launch, every tile
    last = VT_B * VT_H - 1
    first_far_tile = -(-((1 << 32) - last * VT_KT * 8192) // 8192)
    assert 0 < first_far_tile < VT_KT and (last - 1) * VT_KT * 8192 + VT_KT * 8192 <= 1 << 32                        # the last slice is the first that crosses

    g = torch.Generator(device="cuda").manual_seed(77)
    q = torch.randn(VT_B, VT_SQ, VT_H, VT_D, device="cuda", generator=g).to(F8)
    k = torch.empty(VT_B, VT_SK, VT_H, VT_D, dtype=F8, device="cuda")
    v = torch.empty_like(k)
    for b in range(VT_B):                                                 # (per batch entry: the fp32 temporaries stay at 1 GB)
        k[b] = torch.randn(VT_SK, VT_H, VT_D, device="cuda", generator=g).to(F8)
        t = torch.randn(VT_SK, VT_H, VT_D, device="cuda", generator=g)
        t[first_far_tile * 64:] += VT_SHIFT
        v[b] = t.to(F8)
    del t
    ds = {n: (0.5 + torch.rand(VT_B, VT_H, generator=torch.Generator().manual_seed(i))).cuda()
          for i, n in enumerate(("q_descale", "k_descale", "v_descale"))}
    out, lse, *_ = mha_fwd(q, k, v, **ds)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(lse).all())
    for b, h in ((0, 0), (VT_B // 2 - 1, 3), (VT_B - 1, VT_H - 1)):
        qs, ks, vs = [t[b:b + 1, :, h:h + 1].float().cpu() for t in (q, k, v)]
        dss = {n: t[b:b + 1, h:h + 1].cpu() for n, t in ds.items()}
        o_ref, lse_ref, _ = orc.qkskip_fwd(qs, ks, vs, block_m=256, block_n=64, p_round=fp8_p_round(), **dss)
        err_o = (out[b:b + 1, :, h:h + 1].float().cpu() - o_ref).abs().max().item()
        err_l = (lse[b:b + 1, h:h + 1].cpu() - lse_ref).abs().max().item()
        print(f"fp8 V^T past 4 GiB (b, h) = ({b}, {h}): max|o_ref| {o_ref.abs().max().item():.4f} err_o {err_o:.3e} tol {f8._tol(o_ref):.3e} err_lse {err_l:.3e}")
        assert o_ref.abs().max().item() > 0.25 * VT_SHIFT * (VT_KT - first_far_tile) / VT_KT          # the shift is in the result
        assert err_o <= f8._tol(o_ref), (b, h, err_o, f8._tol(o_ref))
        assert err_l <= fp8_lse_tol(), (b, h, err_l)
