"""GPU: layout and neighbour independence of every forward kernel body.

No arithmetic in la_fwd depends on an address, so every case runs one problem twice in one process - *clean* (q, k, v contiguous, `out`
freshly allocated) and *embedded* (q, k, v strided views into larger buffers whose every other element is poison: NaN, the largest finite
value with alternating sign, or infinity; `out` a strided view into a buffer of canary bits, tests/layout_cases.py) - and asserts

* `out`, `lse` and the write list (where there is one) BIT-IDENTICAL between the two runs (torch.equal on the raw 16- / 32-bit patterns),
* every canary element around `out` unchanged,
* the q / k / v buffers, poison included, unchanged byte for byte,
* the clean run within the oracle tolerance the existing test of that body uses (`_tol` and the 1e-3 LSE bound of
  tests/test_gpu_head_dims.py; `_tol` of tests/test_gpu_fp8.py with helpers.fp8_lse_tol(); `_compare_lists` of tests/test_gpu_parity.py),
  so that two equally wrong runs cannot pass. There is no tolerance of this file's own.

What the poison sits in: the rows before row 0 and after the last row of every batch and the columns D .. 2 D of every row (wide_rows);
the rows after a head's last row, followed by the next head (bhsd: head stride > row stride); the rows after the last row of a packed QKV
tensor; the rows before the first and after the last sequence of a packed variable-length batch; the valid rows of key tiles that a read list skips; the
valid rows of a key tile only the OTHER half of a half-vote workgroup lists. These are the rows the kernels clamp, mask, zero or sit out:
the tile-address table and its four-ahead staging, the 128-row template's clamp to the last row with P = 0, the query rows past seqlen_q
replaced by zero rows, the zeros of the fp8 V^T prepare pass, the half-vote activity words.

Shapes are the smallest that reach each guarded path (B = 2, H = 4, Hk = 2: the neighbouring K/V head is not the one a query head reads)."""
import pytest
import torch

import layout_cases as lc
import test_gpu_fp8 as f8
import test_gpu_head_dims as hd
from helpers import fp8_lse_tol, fp8_p_round
from layout_cases import F8
from test_gpu_half_vote import half          # noqa: F401  (fixture: LA_VOTE=half)
from test_gpu_parity import _compare_lists

pytestmark = pytest.mark.gpu
LEAD, TRAIL = 3, 72                           # poison rows before / after: more than one 64-row key tile behind the last row
NEG_INF = float("-inf")

# (id, dtype, head_dim, environment)
BF, HF = torch.bfloat16, torch.float16
BODIES_16 = [(f"{n}-d{D}", dt, D, {}) for D in (64, 96, 128, 192, 256) for n, dt in (("bf16", BF), ("fp16", HF))]
BODIES_V2 = [(f"v2-{n}-d{D}", dt, D, {"LA_FWD_KERNEL": "v2"}) for D in (64, 128, 256) for n, dt in (("bf16", BF), ("fp16", HF))]
BODIES_F8 = [(f"e4m3-d{D}", F8, D, {}) for D in (64, 96, 128, 192, 256)] + \
            [("e4m3-d128-encoded", F8, 128, {"LA_FP8_P": "encoded"}), ("e4m3-d128-mfma_rowsum", F8, 128, {"LA_FP8_P": "mfma_rowsum"})]
BODIES = BODIES_16 + BODIES_V2 + BODIES_F8
BY_ID = {b[0]: b for b in BODIES}
# one 16-bit and one fp8 body per head-dim family (<= 128: 256-row q-tiles; > 128: 128-row q-tiles) for what does not differ between bodies
EXTRA = [BY_ID[i] for i in ("bf16-d128", "fp16-d256", "e4m3-d64", "e4m3-d192")]
SHAPES = [(130, 13), (257, 65), (300, 203)]
B, H, HK = 2, 4, 2


def _ids(bodies):
    return [b[0] for b in bodies]


def _setenv(monkeypatch, body):
    for name in ("LA_FWD_KERNEL", "LA_FP8_P"):
        monkeypatch.delenv(name, raising=False)
    for name, val in body[3].items():
        monkeypatch.setenv(name, val)


def _randn(shape, dtype, g):
    return torch.randn(*shape, generator=g).to(dtype)


def _descales(dtype, nb, hk, g):
    if dtype != F8:
        return {}
    return {n: (0.5 + torch.rand(nb, hk, generator=g)) for n in ("q_descale", "k_descale", "v_descale")}


def _dev(ds):
    return {n: t.cuda() for n, t in ds.items()}


def _check_against_oracle(body, out, lse, q, k, v, ds, lists=None, ulps=0.75):
    """The clean run against the C oracle, under the existing rule of the body: `out` (B, Sq, H, D) and `lse` (B, H, Sq) on the CPU; q, k, v CPU
    tensors. lists = (read list int32, write list of the kernel, must-do row or None): + the write lists (tests/test_gpu_parity.py)."""
    import liteattention_amd as L
    from oracle import oracle as orc
    _, dtype, D, _ = body
    bm, bn = L.get_tile_sizes(D, 1 if dtype == F8 else 2)
    kw = {}
    if lists is not None:
        rd, wr, md = lists
        wr_orc = torch.zeros_like(rd)
        margins = torch.empty(q.shape[0], q.shape[2], rd.shape[2], -(-k.shape[1] // bn))
        kw = dict(read_list=rd, write_list=wr_orc, must_do_list=md, thr=NEG_INF, margins=margins)
    if dtype == F8:
        o_ref, lse_ref, _ = orc.qkskip_fwd(q.float(), k.float(), v.float(), block_m=bm, block_n=bn, p_round=fp8_p_round(), **ds, **kw)
        err_o, err_l = (out.float() - o_ref).abs().max().item(), (lse - lse_ref).abs().max().item()
        assert err_o <= f8._tol(o_ref), (body[0], err_o, f8._tol(o_ref))
        assert err_l <= fp8_lse_tol(), (body[0], err_l)
    else:
        o_ref, lse_ref, _ = orc.qkskip_fwd(q, k, v, block_m=bm, block_n=bn, p_round="f16" if dtype == HF else True, **kw)
        err_o, err_l = (out.float() - o_ref).abs().max().item(), (lse - lse_ref).abs().max().item()
        assert err_o <= hd._tol(o_ref, dtype, ulps=ulps), (body[0], err_o, hd._tol(o_ref, dtype, ulps=ulps))
        assert err_l <= 1e-3, (body[0], err_l)
    if lists is not None:
        bad, _ = _compare_lists(orc, rd, wr, wr_orc, margins, NEG_INF, q.shape[0])
        assert bad == 0


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(lc.raw(a) if a.dtype != torch.float32 else a.view(torch.int32),
                                              lc.raw(b) if b.dtype != torch.float32 else b.view(torch.int32))


def _embedded_equals_clean(launch, clean, bufs, views, out_shape, out_layouts=lc.OUT_LAYOUTS):
    """`launch(q, k, v, out)` -> (out, lse, write list or None) on the views, once per `out` layout; `clean` = the same on contiguous tensors."""
    for out_layout in out_layouts:
        obuf, oview = lc.embed_out(out_shape, torch.bfloat16 if views[0].dtype == F8 else views[0].dtype, out_layout, "cuda", trail=TRAIL)
        before = [lc.raw(b).clone() for b in bufs]
        o, lse, wr = launch(*views, oview)
        torch.cuda.synchronize()
        assert o.data_ptr() == oview.data_ptr() and o.stride() == oview.stride()
        assert _bits_equal(oview, clean[0]), out_layout
        assert _bits_equal(lse, clean[1]), out_layout
        assert (wr is None) == (clean[2] is None) and (wr is None or torch.equal(wr, clean[2])), out_layout
        assert lc.canary_intact(obuf, lc.covered(out_shape, out_layout, 0, TRAIL, device="cuda")), out_layout
        for b, b0 in zip(bufs, before):
            assert torch.equal(lc.raw(b), b0), out_layout


def _embed_qkv(q, k, v, layout, poison):
    """((buffers), (q, k, v views)) on the device; ``batch0``: k and v as one image with batch stride 0, q in wide rows."""
    if layout == "packed_qkv":
        buf, views = lc.embed((q, k, v), layout, poison, LEAD, TRAIL)
        return (buf,), views
    pairs = [lc.embed(t, "wide_rows" if (layout == "batch0" and i == 0) else layout, poison, LEAD, TRAIL) for i, t in enumerate((q, k, v))]
    return tuple(p[0] for p in pairs), tuple(p[1] for p in pairs)


# ------------------------------------------------------------------------------------------------------------------ dense launches
_CLEAN = {}          # (body id, case) -> the clean run, checked against the oracle once: shared by every layout / poison of the case


def _dense_launch(ds):
    from liteattention_amd.flash_attn_interface import mha_fwd

    def launch(q, k, v, out):
        o, lse, *_ = mha_fwd(q, k, v, out=out, **ds)          # default num_splits: one launch, the host split is not taken
        return o, lse, None
    return launch


def _dense_clean(body, Sq, Sk, hk=HK, batch0=False):
    key = (body[0], Sq, Sk, hk, batch0)
    if key not in _CLEAN:
        _, dtype, D, _ = body
        g = torch.Generator().manual_seed(Sq * 7 + Sk + D)
        q = _randn((B, Sq, H, D), dtype, g)
        k, v = [_randn((1 if batch0 else B, Sk, hk, D), dtype, g) for _ in range(2)]
        if batch0:
            k, v = [t.expand(B, Sk, hk, D).contiguous() for t in (k, v)]         # the materialised copy
        ds = _descales(dtype, B, hk, g)
        qd, kd, vd, dsd = q.cuda(), k.cuda(), v.cuda(), _dev(ds)
        o, lse, _ = _dense_launch(dsd)(qd, kd, vd, None)
        assert o.is_contiguous()
        _check_against_oracle(body, o.cpu(), lse.cpu(), q, k, v, ds)
        _CLEAN[key] = (qd, kd, vd, dsd, (o, lse, None))
    return _CLEAN[key]


def _dense_case(monkeypatch, body, shape, layout, poison, hk=HK):
    _setenv(monkeypatch, body)
    Sq, Sk = shape
    qd, kd, vd, dsd, clean = _dense_clean(body, Sq, Sk, hk, batch0=layout == "batch0")
    bufs, views = _embed_qkv(qd, kd, vd, layout, poison)
    assert all(lc.strides_ok(x, body[1] == F8) for x in views)
    _embedded_equals_clean(_dense_launch(dsd), clean, bufs, views, (B, Sq, H, body[2]))


@pytest.mark.parametrize("poison", ["nan", "huge"])
@pytest.mark.parametrize("layout", ["wide_rows", "bhsd"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("body", BODIES, ids=_ids(BODIES))
def test_dense_embedded_equals_clean(monkeypatch, body, shape, layout, poison):
    """Every body, both q / k / v layouts with both `out` layouts. (130, 13): a key sequence shorter than a DMA piece - every row clamped -
    and a q-tile with two valid rows in its second 128 rows; (257, 65): one key in the last tile, one query in the last q-tile;
    (300, 203): ragged on both sides, four key tiles - the four-ahead staging runs past the end of the walk."""
    _dense_case(monkeypatch, body, shape, layout, poison)


PACKED_QKV = [(b, p) for b in EXTRA for p in lc.POISONS if (b[1], p) in lc.POISON_BITS]          # (e4m3fn has no infinity)


@pytest.mark.parametrize("body,poison", PACKED_QKV, ids=[f"{b[0]}-{p}" for b, p in PACKED_QKV])
def test_dense_packed_qkv(monkeypatch, body, poison):
    """q, k, v = the three slices of one (B, S + trail, 3, H, D) tensor: a row's neighbours are the other two operands."""
    _dense_case(monkeypatch, body, (203, 203), "packed_qkv", poison, hk=H)


@pytest.mark.parametrize("poison", ["nan", "huge"])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("body", EXTRA, ids=_ids(EXTRA))
def test_dense_batch_stride_zero(monkeypatch, body, shape, poison):
    """K and V: one image read by every batch entry (batch stride 0; e4m3: through the V^T prepare pass); the clean run reads a copy per entry."""
    _dense_case(monkeypatch, body, shape, "batch0", poison)


@pytest.mark.parametrize("layout", ["wide_rows", "bhsd"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("body", [b for b in EXTRA if b[1] != F8], ids=_ids([b for b in EXTRA if b[1] != F8]))
def test_dense_infinite_neighbours(monkeypatch, body, shape, layout):
    _dense_case(monkeypatch, body, shape, layout, "inf")


# --------------------------------------------------------------------------------------------------------------- packed batches
VARLEN_BODIES = [BY_ID[i] for i in ("bf16-d64", "fp16-d96", "bf16-d128", "fp16-d192", "bf16-d256", "v2-bf16-d128", "e4m3-d64", "e4m3-d128",
                                    "e4m3-d192")]
LENS_Q, LENS_K = [130, 5, 1, 257], [13, 0, 65, 203]


def _cu(lens):
    return torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32)


def _varlen_launch(cu_q, cu_k, ds):
    from liteattention_amd.flash_attn_interface import mha_fwd

    def launch(q, k, v, out):
        o, lse, *_ = mha_fwd(q, k, v, out=out, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, max_seqlen_q=max(LENS_Q), max_seqlen_k=max(LENS_K), **ds)
        return o, lse, None
    return launch


def _varlen_clean(body):
    key = (body[0], "varlen")
    if key not in _CLEAN:
        import liteattention_amd as L
        _, dtype, D, _ = body
        nb = len(LENS_Q)
        g = torch.Generator().manual_seed(D + 5)
        q = _randn((sum(LENS_Q), H, D), dtype, g)
        k, v = [_randn((sum(LENS_K), HK, D), dtype, g) for _ in range(2)]
        ds = _descales(dtype, nb, HK, g)
        cu_q, cu_k = _cu(LENS_Q), _cu(LENS_K)
        qd, kd, vd, dsd, cqd, ckd = q.cuda(), k.cuda(), v.cuda(), _dev(ds), cu_q.cuda(), cu_k.cuda()
        o, lse, _ = L.flash_attn_varlen_func(qd, kd, vd, cqd, ckd, max(LENS_Q), max(LENS_K), return_attn_probs=True, **dsd)
        oc, lc_ = o.cpu(), lse.cpu()
        for b in range(nb):
            q0, q1, k0, k1 = int(cu_q[b]), int(cu_q[b + 1]), int(cu_k[b]), int(cu_k[b + 1])
            if k1 == k0:                                   # the sequence without keys: o = 0, lse = +inf
                assert bool((oc[q0:q1].float() == 0).all()) and bool((lc_[:, q0:q1] == float("inf")).all())
                continue
            _check_against_oracle(body, oc[q0:q1][None], lc_[:, q0:q1][None], q[q0:q1][None], k[k0:k1][None], v[k0:k1][None],
                                  {n: t[b:b + 1] for n, t in ds.items()})
        _CLEAN[key] = (qd, kd, vd, dsd, cqd, ckd, (o, lse, None))
    return _CLEAN[key]


@pytest.mark.parametrize("poison", ["nan", "huge"])
@pytest.mark.parametrize("layout", ["wide_rows", "bhsd"])
@pytest.mark.parametrize("body", VARLEN_BODIES, ids=_ids(VARLEN_BODIES))
def test_packed_batch_embedded_equals_clean(monkeypatch, body, layout, poison):
    """Packed variable-length batch (one launch): key lengths [13, 0, 65, 203], query lengths [130, 5, 1, 257]. The clean run goes through
    ``flash_attn_varlen_func``; the embedded one through the ``mha_fwd`` call that function makes, because only there `out` can be given.

    The ABI cannot express poison rows BETWEEN the sequences: ``seq_view`` (la_kernel_params.h) takes sequence b's length as
    cu[b + 1] - cu[b], so rows inserted behind a sequence would belong to it - the clip to max_seqlen only cuts the longest sequence, which
    is the last one here. So a sequence's row neighbours are the next sequence's rows (ordinary data: a kernel that blends them in fails
    the oracle check of the clean run), and the poison sits before the first and after the last sequence and in the columns D .. 2 D of
    every row (wide_rows), or after the last row of every head, in front of the next head's first sequence (bhsd: (H, T + trail, D))."""
    _setenv(monkeypatch, body)
    qd, kd, vd, dsd, cqd, ckd, clean = _varlen_clean(body)
    pairs = [lc.embed(t, layout, poison, LEAD, TRAIL) for t in (qd, kd, vd)]
    views = tuple(p[1] for p in pairs)
    assert all(lc.strides_ok(x, body[1] == F8) for x in views)
    _embedded_equals_clean(_varlen_launch(cqd, ckd, dsd), clean, tuple(p[0] for p in pairs), views, (sum(LENS_Q), H, body[2]))
    q0 = sum(LENS_Q[:1])
    assert bool((clean[0][q0:q0 + LENS_Q[1]].float() == 0).all()) and bool((clean[1][:, q0:q0 + LENS_Q[1]] == float("inf")).all())


# ---------------------------------------------------------------------------------------------------------------- list launches
LIST_BODIES = [BY_ID[i] for i in ("bf16-d64", "bf16-d128", "bf16-d192", "fp16-d96", "e4m3-d128", "e4m3-d256", "v2-bf16-d128")] + \
              [("bf16-d128-int16", BF, 128, {})]
LB, LH = 1, 2


def _list_launch(rd, md, ds):
    from liteattention_amd.flash_attn_interface import mha_fwd

    def launch(q, k, v, out):
        wr = torch.full_like(rd, -7)
        o, lse, *_ = mha_fwd(q, k, v, out=out, attn_read_list=rd, attn_write_list=wr, attn_must_do_list=md, _must_do_is_1d=md is not None,
                             thr=NEG_INF, **ds)
        return o, lse, wr
    return launch


def _list_clean(body, must_do, Sq=lc.LIST_S, rows=None):
    """The clean launch on the hand-built read lists (every row: tiles 9 8 7 6 | 4 3 | 1 0; thr = -inf, so nothing is dropped), checked against
    the oracle; the write list must be the read list (a fixed point)."""
    key = (body[0], "lists", must_do, Sq)
    if key not in _CLEAN:
        import liteattention_amd as L
        from oracle import oracle as orc
        name, dtype, D, _ = body
        bm, bn = L.get_tile_sizes(D, 1 if dtype == F8 else 2)
        assert bn == 64
        Qt = -(-Sq // bm)
        g = torch.Generator().manual_seed(D + 11)
        q = _randn((LB, Sq, LH, D), dtype, g)
        k, v = [_randn((LB, lc.LIST_S, LH, D), dtype, g) for _ in range(2)]
        ds = _descales(dtype, LB, LH, g)
        rd = lc.list_rows(rows if rows is not None else [lc.LIST_RANGES] * Qt, LB, LH)
        md = orc.expand_must_do_ref(lc.MUST_DO_KEYS, bn, lc.LIST_KT + 1) if must_do else None
        rd_d = rd.to(torch.int16).cuda() if name.endswith("int16") else rd.cuda()
        md_d = None if md is None else md.cuda()
        qd, kd, vd, dsd = q.cuda(), k.cuda(), v.cuda(), _dev(ds)
        o, lse, wr = _list_launch(rd_d, md_d, dsd)(qd, kd, vd, None)
        wr_c = wr.cpu().to(torch.int32)
        _check_against_oracle(body, o.cpu(), lse.cpu(), q, k, v, ds, lists=(rd, wr_c, md), ulps=1.0)    # the rule of test_multi_step_lists_match_oracle
        for m in range(Qt):
            n = int(rd[0, 0, m, 0])
            assert torch.equal(wr_c[:, :, m, :n + 1], rd[:, :, m, :n + 1])
        _CLEAN[key] = (qd, kd, vd, dsd, rd_d, md_d, (o, lse, wr))
    return _CLEAN[key]


@pytest.mark.parametrize("must_do", [False, True], ids=["", "must_do_1d"])
@pytest.mark.parametrize("body", LIST_BODIES, ids=_ids(LIST_BODIES))
def test_list_launch_embedded_equals_clean(monkeypatch, body, must_do):
    """(a) S = 600 (Kt = 10, the last tile of 24 keys; Qt = 3 or 5), read lists of three descending ranges without tiles 2 and 5: out, lse and the
    write list of the embedded launch are the clean launch's bits, in both q / k / v layouts, both `out` layouts and under NaN and huge neighbours."""
    _setenv(monkeypatch, body)
    qd, kd, vd, dsd, rd_d, md_d, clean = _list_clean(body, must_do)
    for layout in ("wide_rows", "bhsd"):
        for poison in ("nan", "huge"):
            bufs, views = _embed_qkv(qd, kd, vd, layout, poison)
            _embedded_equals_clean(_list_launch(rd_d, md_d, dsd), clean, bufs, views, (LB, lc.LIST_S, LH, body[2]))


@pytest.mark.parametrize("poison", ["nan", "huge"])
@pytest.mark.parametrize("body", LIST_BODIES, ids=_ids(LIST_BODIES))
def test_skipped_tiles_are_not_read_into_any_result(monkeypatch, body, poison):
    """(b) Clean layout; the VALID K and V rows of tiles 2 and 5 - which no row lists - overwritten with poison: out, lse and the write list
    are the unpoisoned launch's bits, and finite. Not vacuous: the same poison in a LISTED tile (4) changes the output."""
    _setenv(monkeypatch, body)
    qd, kd, vd, dsd, rd_d, md_d, clean = _list_clean(body, False)
    launch = _list_launch(rd_d, md_d, dsd)
    skipped = [lc.tile_rows(t) for t in lc.SKIPPED_TILES]
    o, lse, wr = launch(qd, lc.poison_rows(kd, skipped, poison), lc.poison_rows(vd, skipped, poison), None)
    assert _bits_equal(o, clean[0]) and _bits_equal(lse, clean[1]) and torch.equal(wr, clean[2])
    assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(lse).all())
    listed = [lc.tile_rows(4)]
    o2, _, _ = launch(qd, lc.poison_rows(kd, listed, poison), lc.poison_rows(vd, listed, poison), None)
    assert not _bits_equal(o2, clean[0])


@pytest.mark.parametrize("poison", ["nan", "huge"])
@pytest.mark.parametrize("D", [128, 64])
def test_half_vote_a_half_sits_out_the_other_halfs_tile(half, D, poison):
    """(c) LA_VOTE=half, Sq = 512: two workgroup items of two 128-row halves each. Tile 7 is listed by half 0 of every item and by no half 1;
    its K and V rows are poison. Every output row, LSE entry and write-list row of every half 1 is the unpoisoned launch's bits - the waves of
    a half sit out the tiles only the other half lists, although the tile is in the workgroup's LDS. Not vacuous: every half 0 differs."""
    body = (f"half-bf16-d{D}", BF, D, {})
    Sq = 512
    qd, kd, vd, dsd, rd_d, md_d, clean = _list_clean(body, False, Sq=Sq, rows=[lc.HALF0_RANGES, lc.HALF1_RANGES] * 2)
    assert rd_d.shape[2] == 4
    tile = [lc.tile_rows(lc.HALF_TILE)]
    o, lse, wr = _list_launch(rd_d, md_d, dsd)(qd, lc.poison_rows(kd, tile, poison), lc.poison_rows(vd, tile, poison), None)
    for m in range(4):
        rows = slice(128 * m, 128 * (m + 1))
        if m % 2 == 1:
            assert _bits_equal(o[:, rows], clean[0][:, rows]) and _bits_equal(lse[:, :, rows], clean[1][:, :, rows]), m
            assert torch.equal(wr[:, :, m], clean[2][:, :, m]), m
        else:
            for h in range(LH):
                assert not _bits_equal(o[:, rows, h], clean[0][:, rows, h]), (m, h)
