"""CPU: the cases of tests/nonfinite_cases.py are what tests/test_gpu_nonfinite.py takes them for.

* every poison kind of every type round-trips as the intended bit pattern;
* the twin differs from the poisoned input only inside the poisoned heads, rows or elements, and both the poisoned and the clean set are
  non-empty in every batch entry;
* the finite / non-finite pattern the GPU test asserts (``a_expectation``, ``nonfinite_masks``) is the pattern of the plain fp64 softmax on
  those exact inputs - every family-A and family-B case at the smallest head dim of each family (64: 256-row q-tiles; 192: 128-row);
* the C oracle keeps the clean heads, rows and columns bit-identical between the poisoned input and the twin, lists included;
* the packed batch alternates poisoned 560-key sequences with clean ones of 13, 65 and 130 keys; every walk length 1 .. 5 and 9 occurs."""
import pytest
import torch

import layout_cases as lc
import nonfinite_cases as nf
from layout_cases import F8

BF, HF = torch.bfloat16, torch.float16
DTYPES = [BF, HF, F8]
DT_IDS = ["bf16", "fp16", "e4m3"]
FAMILIES = [(64, 256), (192, 128)]                 # (smallest head dim of the family, rows of its q-tile)
NB = 2                                             # batch entries of the CPU check: the first entries of any larger batch (a_base)
NEG_INF = float("-inf")


def _p_rounds(dtype):
    return {BF: (True,), HF: ("f16",), F8: ("fp8", "fp8_lin")}[dtype]


def _oracle(q, k, v, ds, bm, p_round, **kw):
    from oracle import oracle as orc
    f = (lambda x: x.float()) if q.dtype == F8 else (lambda x: x)
    return orc.qkskip_fwd(f(q), f(k), f(v), block_m=bm, block_n=nf.BN, p_round=p_round, **ds, **kw)


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


_BASE = {}


def _base(D):
    if D not in _BASE:
        _BASE[D] = nf.a_base(D, NB, DTYPES)
    return _BASE[D]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_poison_patterns_round_trip(dtype):
    big = {BF: 3.3895313892515355e38, HF: 65504.0, F8: 448.0}[dtype]
    assert nf.kinds(dtype) == (["nan", "huge"] if dtype == F8 else ["nan", "inf", "huge"])
    for kind in nf.kinds(dtype):
        pat = nf.pattern(dtype, kind, 8)
        bits = [b & (0xFF if dtype == F8 else 0xFFFF) for b in pat.tolist()]
        assert bits == list(lc.POISON_BITS[(dtype, kind)]) * 4
        x = pat.view(dtype).float()
        if kind == "nan":
            assert bool(torch.isnan(x).all())
        elif kind == "inf":
            assert x.tolist() == [float("inf"), NEG_INF] * 4
        else:
            assert x.tolist() == [big, -big] * 4
        # ... and through the helpers that place it
        t = torch.zeros(NB, 3, nf.A_HK, 8).to(dtype)
        m = nf.a_poisoned_kv(NB)
        p = nf.poison_heads(t, m, kind)
        assert torch.equal(lc.raw(p)[m[:, None, :, None].expand(p.shape)].view(-1, 8), pat.expand(NB * 3, 8))
        assert bool((lc.raw(p)[~m[:, None, :, None].expand(p.shape)] == 0).all())


def test_poisoned_sets_are_a_seeded_half_and_never_empty():
    for B in (2, 7, 96, 192):
        kv, qh = nf.a_poisoned_kv(B), nf.a_poisoned_q(B)
        assert bool((kv.sum(1) == 1).all()) and bool((qh.sum(1) == 2).all())               # half of the pairs; neither set empty in any entry
        assert torch.equal(kv, nf.a_poisoned_kv(B)) and torch.equal(qh, nf.a_poisoned_q(B))
        assert torch.equal(nf.a_poisoned_heads("kv", B), kv.repeat_interleave(2, dim=1))
        if B >= 96:
            assert 0.25 < kv[:, 0].float().mean().item() < 0.75                             # not one fixed head
    assert nf.A_H == 2 * nf.A_HK


def test_base_entries_do_not_depend_on_the_batch():
    small, large = nf.a_base(64, 2, [BF, F8]), nf.a_base(64, 3, [BF, F8])
    for dt in (BF, F8):
        for a, b in zip(small[dt][:3], large[dt][:3]):
            assert torch.equal(lc.raw(a), lc.raw(b[:2])) and bool(torch.isfinite(a.float()).all())
    assert torch.equal(small[F8][3]["k_descale"], large[F8][3]["k_descale"][:2]) and small[BF][3] == {}


def test_expectations():
    for target in nf.A_TARGETS:
        assert nf.a_expectation(target, "inf") is None and nf.a_expectation(target, "huge", encoded=True) is None
        assert nf.a_expectation(target, "nan") == nf.Expect("nonfinite", "twin" if target == "v" else "nonfinite")
        # the byte-encoded P drops a key with a NaN score (hardware conversion): V alone is as everywhere
        assert nf.a_expectation(target, "nan", encoded=True) == \
            {"v": nf.a_expectation("v", "nan"), "kv": nf.Expect("nonfinite", "neg_inf")}.get(target, nf.Expect("zero", "neg_inf"))


def test_walk_lengths():
    assert [nf.walk_len(s) for s in nf.A_KEY_LENS] == [1, 1, 2, 3, 4, 5, 9]
    assert {nf.walk_len(s) for s in nf.A_KEY_LENS} == {1, 2, 3, 4, 5, 9}
    assert all(s % nf.BN for s in nf.A_KEY_LENS)                                           # every tail is ragged
    assert nf.a_seqlen_q(256) == 300 and nf.a_seqlen_q(128) == 172 and nf.A_SQ_MAX == 300
    assert nf.walk_len(nf.A_SK_MAX) == lc.LIST_KT and nf.walk_len(nf.B_SK) == 4


def _check_heads(dtype, bm, q, k, v, ds, target, kind, keys=None, lists=None):
    """One family-A case: the twin differs inside the poisoned heads only; the fp64 softmax gives the asserted pattern; the oracle keeps
    the clean heads bit-identical."""
    B = q.shape[0]
    qp, kp, vp = nf.a_poison(q, k, v, target, kind)
    heads = nf.a_poisoned_heads(target, B)
    assert bool(heads.any(1).all()) and bool((~heads).any(1).all())
    for t, tp, name in ((q, qp, "q"), (k, kp, "k"), (v, vp, "v")):
        diff = (lc.raw(t) != lc.raw(tp)).any(3).any(1)                                       # (B, heads of t)
        want = (nf.a_poisoned_q(B) if name == "q" else nf.a_poisoned_kv(B)) if name in target else torch.zeros_like(diff)
        assert torch.equal(diff, want), (name, target)
        if name in target:                                                                 # EVERY element of those heads is poison
            pat = nf.pattern(dtype, kind, t.shape[-1])
            assert bool((lc.raw(tp).permute(0, 2, 1, 3)[want] == pat).all())
    bad_o, bad_l = nf.nonfinite_masks(qp, kp, vp, ds, keys=keys)
    assert not bool(bad_o.permute(0, 2, 1, 3)[~heads].any()) and not bool(bad_l[~heads].any())          # clean heads: finite
    exp = nf.a_expectation(target, kind)
    if exp is not None:
        assert bool(bad_o.permute(0, 2, 1, 3)[heads].all()) and exp.out == "nonfinite"
        assert bool(bad_l[heads].all()) == (exp.lse == "nonfinite") and bool(bad_l[heads].any()) == (exp.lse == "nonfinite")
    for p_round in _p_rounds(dtype):
        thrs = (None,) if lists is None else (NEG_INF, nf.FINITE_THR)
        for thr in thrs:
            kw, kwp, wr, wrp = {}, {}, None, None
            if lists is not None:
                wr, wrp = torch.full_like(lists, -7), torch.full_like(lists, -7)
                kw, kwp = dict(read_list=lists, write_list=wr, thr=thr), dict(read_list=lists, write_list=wrp, thr=thr)
            o, lse, _ = _oracle(q, k, v, ds, bm, p_round, **kw)
            op, lsep, _ = _oracle(qp, kp, vp, ds, bm, p_round, **kwp)
            assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(lse).all())
            assert _same(o.permute(0, 2, 1, 3)[~heads], op.permute(0, 2, 1, 3)[~heads]) and _same(lse[~heads], lsep[~heads]), (target, kind, p_round)
            if lists is not None:
                assert torch.equal(wr[~heads], wrp[~heads])
            if exp is not None and exp.lse == "twin":
                assert _same(lse, lsep)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("D,bm", FAMILIES, ids=["d64", "d192"])
def test_family_a_dense_cases(D, bm, dtype):
    q0, k0, v0, ds = _base(D)[dtype]
    for Sk in nf.A_KEY_LENS:
        q, k, v = q0[:, :nf.a_seqlen_q(bm)], k0[:, :Sk], v0[:, :Sk]
        for target in nf.A_TARGETS:
            for kind in nf.kinds(dtype):
                _check_heads(dtype, bm, q, k, v, ds, target, kind)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("D,bm", FAMILIES, ids=["d64", "d192"])
def test_family_a_list_cases(D, bm, dtype):
    from oracle import oracle as orc
    q0, k0, v0, ds = _base(D)[dtype]
    Sq = nf.a_seqlen_q(bm)
    rd = lc.list_rows([lc.LIST_RANGES] * 2, NB, nf.A_H)
    walked = orc.walk_tiles(rd[0, 0, 0].tolist())
    keys = torch.zeros(nf.A_SK_MAX, dtype=torch.bool)
    for t in walked:
        keys[lc.tile_rows(t)] = True
    assert -(-Sq // bm) == 2 and not bool(keys[lc.tile_rows(2)].any())
    for target in nf.A_TARGETS:
        for kind in nf.kinds(dtype):
            _check_heads(dtype, bm, q0[:, :Sq], k0, v0, ds, target, kind, keys=keys, lists=rd)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_packed_batch_alternates(dtype):
    n = 8
    lens, flags = nf.packed_lens(n)
    assert lens == [560, 13, 560, 65, 560, 130, 560, 13] and flags == [True, False] * 4
    assert {nf.walk_len(x) for x in lens} == {9, 1, 2, 3}                                   # a nine-tile item, then one that rewrites few ring slots
    q0, k0, v0, ds = nf.a_base(64, n, [dtype])[dtype]
    k = nf.pack(k0, lens)
    rows = nf.packed_row_mask(lens, flags)
    assert k.shape[0] == sum(lens) == int(nf.cu(lens)[-1]) and int(rows.sum()) == 4 * 560
    assert torch.equal(lc.raw(k[560:573]), lc.raw(k0[1, :13]))
    for kind in nf.kinds(dtype):
        kp = nf.poison_packed_rows(k, rows, kind)
        assert torch.equal(lc.raw(kp)[~rows], lc.raw(k)[~rows])
        assert bool((lc.raw(kp)[rows] == nf.pattern(dtype, kind, 64)).all())
    # per sequence the fp64 softmax says: poisoned sequences (K and V, K, or V NaN) as a_expectation, clean ones finite
    Sq = nf.a_seqlen_q(256)
    for target in ("k", "v", "kv"):
        kp = nf.poison_packed_rows(k, rows, "nan") if "k" in target else k
        vp = nf.poison_packed_rows(nf.pack(v0, lens), rows, "nan") if "v" in target else nf.pack(v0, lens)
        c = nf.cu(lens).tolist()
        for b in (0, 1, 2, 3):
            dsb = {name: t[b:b + 1] for name, t in ds.items()}
            bad_o, bad_l = nf.nonfinite_masks(q0[b:b + 1, :Sq], kp[c[b]:c[b + 1]][None], vp[c[b]:c[b + 1]][None], dsb)
            exp = nf.a_expectation(target, "nan")
            if flags[b]:
                assert bool(bad_o.all()) and bool(bad_l.all()) == (exp.lse == "nonfinite") == bool(bad_l.any())
            else:
                assert not bool(bad_o.any()) and not bool(bad_l.any())


# ------------------------------------------------------------------------------------------------------------------ family B
def _b_variants():
    return [(None, None), (nf.b_listed_keys(), lc.list_rows([nf.B_LIST_RANGES] * 3, nf.B_B, nf.B_H, k_tiles=4))]


def _b_oracle(q, k, v, ds, bm, p_round, rd):
    if rd is None:
        return (*_oracle(q, k, v, ds, bm, p_round)[:2], None)
    rd = rd[:, :, :-(-nf.B_SQ // bm)].contiguous()
    wr = torch.full_like(rd, -7)
    o, lse, _ = _oracle(q, k, v, ds, bm, p_round, read_list=rd, write_list=wr, thr=NEG_INF)
    return o, lse, wr


def test_family_b_lists_walk_every_poisoned_key():
    keys = nf.b_listed_keys()
    assert int(keys.sum()) == 64 + 64 + (nf.B_SK - 192) and not bool(keys[128:192].any())
    assert all(bool(keys[key]) for key, _ in nf.b1_positions(64)) and bool(keys[nf.B3_KEY])
    assert [key // nf.BN for key, _ in nf.b1_positions(64)] == [3, 1, 0]                     # last (ragged) tile, a middle one, the first


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("D,bm", FAMILIES, ids=["d64", "d192"])
def test_family_b_cases(D, bm, dtype):
    q, k, v, ds = nf.b_inputs(dtype, D)
    on_kv = nf.b_heads_on_kv()
    assert int(on_kv.sum()) == 2 and bool(on_kv[nf.B_BATCH, nf.B_Q_HEAD])
    cols = [c for _, c in nf.b1_positions(D)]
    assert cols == [0, D - 1, D // 2]
    for keys, rd in _b_variants():
        clean = {p: _b_oracle(q, k, v, ds, bm, p, rd) for p in _p_rounds(dtype)}
        bad_o, bad_l = nf.nonfinite_masks(q, k, v, ds, keys=keys)
        assert not bool(bad_o.any()) and not bool(bad_l.any())
        # B1: three V elements
        for kind in nf.kinds(dtype):
            vp = nf.b1_poison_v(v, kind)
            diff = (lc.raw(vp) != lc.raw(v)).nonzero().tolist()
            assert sorted(diff) == sorted([nf.B_BATCH, key, nf.B_KV_HEAD, c] for key, c in nf.b1_positions(D))
            bad_o, bad_l = nf.nonfinite_masks(q, k, vp, ds, keys=keys)
            want = torch.zeros_like(bad_o)
            if kind != "huge":
                want.permute(0, 2, 1, 3)[on_kv] = torch.zeros(D, dtype=torch.bool).index_fill(0, torch.tensor(cols), True)
            assert torch.equal(bad_o, want) and not bool(bad_l.any()), kind
            other = torch.ones(D, dtype=torch.bool).index_fill(0, torch.tensor(cols), False)
            for p, (o, lse, wr) in clean.items():
                op, lsep, wrp = _b_oracle(q, k, vp, ds, bm, p, rd)
                assert _same(op[..., other].contiguous(), o[..., other].contiguous()) and _same(lsep, lse)
                assert wr is None or torch.equal(wr, wrp)
        # B2: three query rows
        rows = torch.zeros(nf.B_SQ, dtype=torch.bool).index_fill(0, torch.tensor(nf.B2_ROWS), True)
        for kind in nf.kinds(dtype):
            qp = nf.b2_poison_q(q, kind)
            diff = (lc.raw(qp) != lc.raw(q)).any(-1)
            want_rows = torch.zeros_like(diff)
            want_rows[nf.B_BATCH, :, nf.B_Q_HEAD] = rows
            assert torch.equal(diff, want_rows)
            bad_o, bad_l = nf.nonfinite_masks(qp, k, v, ds, keys=keys)
            assert not bool(bad_o[~want_rows].any()) and not bool(bad_l[~want_rows.permute(0, 2, 1)].any())
            if kind == "nan":
                assert bool(bad_o[want_rows].all()) and bool(bad_l[want_rows.permute(0, 2, 1)].all())
            for p, (o, lse, wr) in clean.items():
                op, lsep, wrp = _b_oracle(qp, k, v, ds, bm, p, rd)
                if p != "fp8_lin":              # (the encoded form shares one lazy reference maximum among 64 rows: the GPU test asks the tolerance there)
                    assert _same(op[~want_rows], o[~want_rows]) and _same(lsep[~want_rows.permute(0, 2, 1)], lse[~want_rows.permute(0, 2, 1)])
                head = torch.ones(nf.B_B, nf.B_H, dtype=torch.bool)
                head[nf.B_BATCH, nf.B_Q_HEAD] = False
                assert _same(op.permute(0, 2, 1, 3)[head], o.permute(0, 2, 1, 3)[head]) and _same(lsep[head], lse[head])
                assert wr is None or torch.equal(wr, wrp)
        # B3: one key row
        kp = nf.b3_poison_k(k)
        diff = (lc.raw(kp) != lc.raw(k)).any(-1).nonzero().tolist()
        assert diff == [[nf.B_BATCH, nf.B3_KEY, nf.B_KV_HEAD]]
        bad_o, bad_l = nf.nonfinite_masks(q, kp, v, ds, keys=keys)
        assert torch.equal(bad_l, on_kv[:, :, None].expand_as(bad_l)) and torch.equal(bad_o, on_kv[:, None, :, None].expand_as(bad_o))
        for p, (o, lse, wr) in clean.items():
            op, lsep, _ = _b_oracle(q, kp, v, ds, bm, p, rd)
            assert _same(op.permute(0, 2, 1, 3)[~on_kv], o.permute(0, 2, 1, 3)[~on_kv]) and _same(lsep[~on_kv], lse[~on_kv])


@pytest.mark.parametrize("dtype", [torch.float32, BF, HF], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("which", ["lse", "out"])
def test_merge_cases(which, dtype):
    """The merge reference on one NaN: a NaN LSE makes the merged LSE of its row NaN (and zeroes the row's weights, so the merged output
    is 0: finite); a NaN partial-output element makes that element of the merged output NaN and nothing else."""
    from oracle import oracle as orc
    o, lse = nf.combine_partials(dtype)
    assert lse.stride(-2) == 1 and tuple(lse.shape) == (nf.C_SPLITS, nf.C_B, nf.C_S, nf.C_H)
    op, lsep, (b, s, h) = nf.combine_poison(o, lse, which)
    assert lsep.stride(-2) == 1
    assert int((lc.raw(op) != lc.raw(o)).sum() if dtype != torch.float32 else (op.view(torch.int32) != o.view(torch.int32)).sum()) == (which == "out")
    assert int((lsep.view(torch.int32) != lse.view(torch.int32)).sum()) == (which == "lse")
    ref, lse_ref = orc.attention_combine_ref(o.float(), lse)
    refp, lse_refp = orc.attention_combine_ref(op.float(), lsep)
    row = torch.zeros(nf.C_B, nf.C_S, nf.C_H, dtype=torch.bool)
    row[b, s, h] = True
    assert torch.equal(refp[~row], ref[~row]) and torch.equal(lse_refp[~row], lse_ref[~row])
    if which == "lse":
        assert bool(torch.isnan(lse_refp[row]).all()) and bool(torch.isfinite(refp[row]).all())
    else:
        bad = ~torch.isfinite(refp[b, s, h])
        assert bad.nonzero().tolist() == [[nf.C_OUT_AT[4]]] and bool(torch.isfinite(lse_refp).all())
