"""CPU: the full-size result checker (tools/selfcheck.py) held to the pinned oracle (oracle/).

At B=1, S=75 600, H=40 the CPU oracle cannot finish, so those launches are judged by tools/selfcheck.py: a plain-torch restatement of
the reader, the skip vote and the list writer. Nothing else ties that restatement to the oracle, and nothing shows that it rejects a
wrong result. This file does both, on the CPU:

  a. the row functions (walk_of_row, written_row, lists_to_bitmap, listed_key_mask) against oracle.walk_tiles / simulate_writer on
     seeded random well-formed rows, and on the ill-formed rows where the two used to differ;
  b. the workload functions (banded_rows, listed_tiles_of_rows, executed_flops) against brute force and the oracle, at the headline
     geometry;
  c. sampled_row_check / vote_writer_check ACCEPT the oracle's own O, LSE and write list on fragmented lists;
  d. they REJECT host-made mutations of that result. Every mutation is first sized from an fp32 reference alone and used only where
     it moves the judged quantity by at least 10x the bound in force (asserted): a mutation the bound could not see proves nothing.

Bounds: sampled_row_check's defaults for bf16 / fp16 (|O - ref| <= 2^-8 max|ref| + 1e-4, |LSE - ref| <= 2e-4); for e4m3 the bounds
tests/test_gpu_headline.py uses for the default fp8 form (0.05 max|ref| + 1e-3, 2e-4).
"""
import functools
import itertools
import math
import random

import pytest
import torch

from helpers import fragmented_qkv

F8 = torch.float8_e4m3fn
LN2 = math.log(2.0)


def _orc():
    from oracle import oracle as orc
    return orc


def _sc():
    from tools import selfcheck as sc
    return sc


# ============================================================================================================== a. row functions
def _row_of_bitmap(keep):
    """[L, start0, end0, ...] (descending inclusive ranges) of a list of booleans over tiles 0 .. kt-1; written here on its own."""
    row, t = [], len(keep) - 1
    while t >= 0:
        if keep[t]:
            start = t
            while t > 0 and keep[t - 1]:
                t -= 1
            row += [start, t]
        t -= 1
    return [len(row)] + row


def _random_read_row(kt, rng):
    """A well-formed read row: descending disjoint ranges, first start kt - 1, even L. The density of kept tiles and of range breaks
    varies, so rows go from one range to alternating single tiles."""
    p = rng.choice([0.1, 0.3, 0.5, 0.7, 0.9])
    style = rng.random()
    if style < 0.1:
        keep = [True] * kt
    elif style < 0.2:
        keep = [(kt - 1 - t) % 2 == 0 for t in range(kt)]                   # alternating: ceil(kt / 2) single-tile ranges
    else:
        keep = [rng.random() < p for _ in range(kt)]
    keep[kt - 1] = True
    return _row_of_bitmap(keep)


def _fit(row, kt):
    """The row as it sits in a list of kt + 1 entries: zero padded; an entry that would lie behind the row is counted in L and not
    stored (an odd kt with alternating tiles: the last end, 0, is cut off)."""
    return (row + [0] * (kt + 1))[: kt + 1]


def _random_must_do_row(kt, rng):
    """A well-formed must-do row of kt + 1 entries: descending disjoint ranges, a tile n is must-do when end < n <= start; the live
    pairs lie inside the row. From no must-do tile at all ([2, 0, 0]) to several ranges."""
    if kt < 3 or rng.random() < 0.15:
        return _fit([2, 0, 0], kt)
    n_max = max(1, min(6, (kt - 1) // 2))
    cuts = sorted(rng.sample(range(0, kt + 1), min(kt + 1, 2 * rng.randint(1, n_max))), reverse=True)
    cuts = cuts[: len(cuts) // 2 * 2]
    row = [len(cuts)] + cuts
    assert len(row) <= kt + 1
    return _fit(row, kt)


def _kts(n, rng):
    """Key-tile counts from 1 up; one in eight is large enough for rows of more than 64 ranges."""
    for i in range(n):
        if i % 8 == 0:
            yield rng.randint(130, 200)
        elif i % 8 == 1:
            yield rng.randint(1, 4)
        else:
            yield rng.randint(1, 48)


def test_row_functions_equal_the_oracle_on_random_well_formed_rows():
    """6 000 seeded rows: walk_of_row == walk_tiles, written_row == simulate_writer, without and with a random must-do row."""
    orc, sc = _orc(), _sc()
    rng = random.Random(20240611)
    n_rows, longest, cut_off, kt1, multi_md, md_mattered = 6000, 0, 0, 0, 0, 0
    for kt in _kts(n_rows, rng):
        row = _random_read_row(kt, rng)
        longest = max(longest, row[0] // 2)
        assert row[0] % 2 == 0 and row[1] == kt - 1
        cut_off += len(row) > kt + 1
        kt1 += kt == 1
        row = _fit(row, kt)
        walk = orc.walk_tiles(row)
        assert sc.walk_of_row(row) == walk, row
        assert walk[0] == kt - 1 and all(a > b for a, b in zip(walk, walk[1:])), row
        flags = [rng.random() < rng.choice([0.2, 0.5, 0.8]) for _ in walk]       # flags[0] too: the writer must ignore it
        plain = orc.simulate_writer(row, flags)
        assert sc.written_row(row, flags) == plain, (row, flags)
        md = _random_must_do_row(kt, rng)
        multi_md += md[0] >= 4
        with_md = orc.simulate_writer(row, flags, md)
        assert sc.written_row(row, flags, md) == with_md, (row, flags, md)
        assert sc.written_row(row, flags, torch.tensor(md, dtype=torch.int32)) == with_md
        md_mattered += with_md != plain
    assert longest > 64 and cut_off >= 10 and kt1 >= 50 and multi_md >= 1000 and md_mattered >= 500, \
        (longest, cut_off, kt1, multi_md, md_mattered)


# (row, flags, walk, written row): the oracle's answers, recorded. Rows 2 and 3 are the ill-formed rows on which the checker used to differ
# from the oracle (an odd L loads the pair that starts at entry L; a range that walks nothing closes with the vote carried over from
# the tile before it), row 0 is the one-tile row that used to raise IndexError, row 1 the L == 0 row whose first range is still walked.
EXPLICIT_ROWS = [
    ([2, 0], [False], [0], [2, 0, 0]),
    ([0, 5, 3, 1, 0, 0], [False, True, False], [5, 4, 3], [4, 5, 4, 3, 3]),
    ([3, 5, 3, 1, 0, 0], [False, True, False, True, False], [5, 4, 3, 1, 0], [6, 5, 4, 3, 3, 0, 0]),
    ([4, 5, 3, 1, 2, 0], [False, True, True], [5, 4, 3], [2, 5, 4]),
    ([4, 5, 3, 1, 2, 0], [False, False, False], [5, 4, 3], [3, 5, 3, 2]),
    # odd kt, alternating tiles: the last end is cut off (L = kt + 1 counted, kt entries stored) ...
    ([6, 4, 4, 2, 2, 0], [False, False, False], [4, 2, 0], [6, 4, 4, 2, 2, 0, 0]),
    # ... and the same row as the writer stores it back: L capped at kt, so L is odd
    ([5, 4, 4, 2, 2, 0], [True, True, False], [4, 2, 0], [4, 4, 4, 0, 0]),
]


@pytest.mark.parametrize("row,flags,walk,written", EXPLICIT_ROWS)
def test_explicit_rows_follow_the_oracle(row, flags, walk, written):
    orc, sc = _orc(), _sc()
    assert orc.walk_tiles(row) == walk and orc.simulate_writer(row, flags) == written       # the recorded answers are the oracle's
    assert sc.walk_of_row(row) == walk
    assert sc.written_row(row, flags) == written
    kt = len(row) - 1
    bits = sc.lists_to_bitmap(torch.tensor([row], dtype=torch.int32))[0].tolist()
    assert bits == [t in set(walk) for t in range(kt)]
    mask = sc.listed_key_mask(row, 4, 4 * kt - 1, "cpu").tolist()
    assert mask == [k // 4 in set(walk) for k in range(4 * kt - 1)]


def test_stored_row_caps_a_row_at_its_width():
    sc = _sc()
    assert sc.stored_row([2, 0, 0], 1) == [1, 0]                        # one key tile: [L, start] only, L capped at k_tiles
    assert sc.stored_row([6, 4, 4, 2, 2, 0, 0], 5) == [5, 4, 4, 2, 2, 0]
    assert sc.stored_row([4, 5, 4, 3, 3], 6) == [4, 5, 4, 3, 3]


@pytest.mark.parametrize("dtype", [torch.int32, torch.int16])
@pytest.mark.parametrize("kt", [1, 2, 7, 24, 33, 150])
def test_lists_to_bitmap_equals_the_oracles_walk(dtype, kt):
    orc, sc = _orc(), _sc()
    rng = random.Random(kt)
    rows = [_fit(_random_read_row(kt, rng), kt) for _ in range(60)]
    rows.append(_fit([0, kt - 1, max(0, kt - 3)], kt))                  # L == 0: the first range is walked all the same
    rows.append(_fit(_row_of_bitmap([(kt - 1 - t) % 2 == 0 for t in range(kt)]), kt))
    capped = list(rows[-1])
    capped[0] = min(capped[0], kt)                                       # as the writer stores it (odd L when kt is odd)
    rows.append(capped)
    lists = torch.tensor(rows, dtype=dtype).view(3, -1, kt + 1)
    bits = sc.lists_to_bitmap(lists)
    assert bits.shape == (3, lists.shape[1], kt) and bits.dtype == torch.bool
    for got, row in zip(bits.view(-1, kt).tolist(), rows):
        walked = set(orc.walk_tiles(row))
        assert got == [t in walked for t in range(kt)], row


@pytest.mark.parametrize("kt,block_n,cut", [(1, 64, 0), (1, 64, 63), (2, 16, 5), (9, 16, 15), (24, 64, 36), (33, 8, 1), (40, 64, 0)])
def test_listed_key_mask_is_the_bitmap_expanded_to_keys(kt, block_n, cut):
    orc, sc = _orc(), _sc()
    rng = random.Random(100 + kt)
    seqlen_k = kt * block_n - cut                                        # cut > 0: a ragged last tile
    for _ in range(40):
        row = _fit(_random_read_row(kt, rng), kt)
        walked = set(orc.walk_tiles(row))
        want = torch.tensor([t in walked for t in range(kt)]).repeat_interleave(block_n)[:seqlen_k]
        got = sc.listed_key_mask(row, block_n, seqlen_k, "cpu")
        assert got.shape == (seqlen_k,) and torch.equal(got, want), row
        assert torch.equal(want, sc.lists_to_bitmap(torch.tensor(row, dtype=torch.int32)).repeat_interleave(block_n)[:seqlen_k])


# ============================================================================================================== b. workload functions
HEADLINE_S = 75600
GEOMETRIES = [(HEADLINE_S, HEADLINE_S, 256, 64), (HEADLINE_S, HEADLINE_S, 128, 64),
              (300, 330, 64, 16), (1000, 517, 128, 64), (77, 1300, 32, 64), (513, 129, 256, 64)]
SPARSITIES = [0.0, 0.21, 0.42, 0.57, 0.77, 0.9995]


@pytest.mark.parametrize("S,Sk,bm,bn", GEOMETRIES)
@pytest.mark.parametrize("sparsity", SPARSITIES)
def test_banded_rows_and_their_counts(S, Sk, bm, bn, sparsity):
    orc, sc = _orc(), _sc()
    qt, kt = -(-S // bm), -(-Sk // bn)
    if S == HEADLINE_S:
        assert (qt, kt) == ((296, 1182) if bm == 256 else (591, 1182))
    rows = sc.banded_rows(qt, kt, bm, bn, sparsity)
    assert rows.shape == (qt, 5) and rows.dtype == torch.int32
    if sparsity == 0.9995:
        assert round((1.0 - sparsity) * kt) <= 1                         # the band <= 0 branch: only the first walked tile is kept
    total = 0
    for r in rows.tolist():
        walk = orc.walk_tiles(r)
        assert sc.walk_of_row(r) == walk
        assert walk[0] == kt - 1 and walk[-1] >= 0 and all(a > b for a, b in zip(walk, walk[1:])), r      # descending, no overlap
        assert r[0] in (2, 4) and (r[0] == 2 or r[2] > r[3] + 1), r                                        # two ranges never touch
        assert abs(len(walk) - (1.0 - sparsity) * kt) <= 1.0, (r, len(walk))                              # kept share, one tile per row
        total += len(walk)
    assert sc.listed_tiles_of_rows(rows) == total == orc.listed_tiles(rows)
    # executed_flops against the sum over the bitmap of 4 rows cols D, edge tiles at their real size in q and in k
    D, heads, batch = 128, 3, 2
    wide = torch.zeros(qt, kt + 1, dtype=torch.int32)
    wide[:, : min(5, kt + 1)] = rows[:, : kt + 1]
    bits = sc.lists_to_bitmap(wide).to(torch.float64)
    n_rows = torch.tensor([min(bm, S - m * bm) for m in range(qt)], dtype=torch.float64)
    n_cols = torch.tensor([min(bn, Sk - n * bn) for n in range(kt)], dtype=torch.float64)
    brute = 4.0 * D * heads * batch * float((n_rows[:, None] * n_cols[None, :] * bits).sum())
    assert sc.executed_flops(rows, heads, batch, S, Sk, bm, bn, D) == pytest.approx(brute, rel=1e-12)


def test_the_oracle_computes_exactly_the_listed_tiles_of_imposed_rows():
    orc, sc = _orc(), _sc()
    B, H, S, Sk, bm, bn, D = 2, 2, 300, 330, 64, 16, 16
    qt, kt = -(-S // bm), -(-Sk // bn)
    g = torch.Generator().manual_seed(3)
    q, k, v = torch.randn(B, S, H, D, generator=g), torch.randn(B, Sk, H, D, generator=g), torch.randn(B, Sk, H, D, generator=g)
    for sparsity in (0.0, 0.42, 0.77, 0.99):
        rows = sc.banded_rows(qt, kt, bm, bn, sparsity)
        read = torch.zeros(B, H, qt, kt + 1, dtype=torch.int32)
        read[..., :5] = rows
        o, lse, n_tiles = orc.qkskip_fwd(q, k, v, block_m=bm, block_n=bn, read_list=read, thr=float("-inf"), p_round=False)
        assert n_tiles == sc.listed_tiles_of_rows(rows) * B * H
        res = sc.sampled_row_check(q, k, v, o, lse, read, bm, bn, heads=range(H), n_rows=S + 8, batch=1)
        assert res["ok"] and res["rows"] == H * S, res


# ============================================================================================================== c / d. the two verdicts
def gqa_heads(x, group):
    """(B, S, Hk, D) -> (B, S, Hk * group, D): query head h = hk * group + j is head hk's rows rolled by 7 j along the sequence (the
    generator's rows are exchangeable), so the heads of a group differ and every one still lines up with K/V head h // group."""
    return torch.stack([x[:, :, hk].roll(7 * j, dims=1) for hk in range(x.shape[2]) for j in range(group)], dim=2).contiguous()


CASES = {
    # name: dtype, block_m, block_n, Sq, Sk, H, Hk, D, must-do tokens (descending pairs, as LiteAttention takes them)
    "bf16-256": ("bf16", 256, 64, 1500, 1500, 2, 2, 128, None),
    "bf16-128": ("bf16", 128, 64, 1500, 1500, 2, 2, 128, None),
    "fp16-256": ("fp16", 256, 64, 1500, 1500, 2, 2, 128, None),
    "e4m3-256": ("e4m3", 256, 64, 1500, 1500, 2, 2, 128, None),
    "gqa-4-2": ("bf16", 256, 64, 1100, 1487, 4, 2, 128, None),                 # Sq != Sk, both ragged
    "short-last-q-tile": ("bf16", 256, 64, 1300, 1500, 2, 2, 128, None),        # the last q-tile holds 20 rows
    "d64": ("bf16", 128, 64, 1500, 1500, 2, 2, 64, None),
    "must-do": ("bf16", 256, 64, 1500, 1500, 2, 2, 128, (1300, 1000, 700, 450, 200, 0)),
}
STEPS, THR, MIN_RANGES = 3, -3.0, 4       # the generator heats every 3rd or 4th of the 24 key tiles: ~6 ranges per row; 4 is "fragmented"


def _cast(dtype):
    return {"bf16": lambda x: x.bfloat16(), "fp16": lambda x: x.half(), "e4m3": lambda x: x.to(F8)}[dtype]


def _bounds(dtype):
    return dict(o_rtol=0.05, o_atol=1e-3, lse_atol=2e-4) if dtype == "e4m3" else dict(o_rtol=2.0 ** -8, o_atol=1e-4, lse_atol=2e-4)


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """The oracle's own result on the fragmenting generator over STEPS ping-pong steps: per step q, k, v (in the case's dtype), O rounded
    to the output dtype (e4m3 inputs return bf16), LSE, the read and the written list and the oracle's decision margins."""
    orc = _orc()
    dtype, bm, bn, Sq, Sk, H, Hk, D, md_tokens = CASES[name]
    B = 1
    qt, kt = -(-Sq // bm), -(-Sk // bn)
    lists = orc.init_skip_list_ref(B, qt, kt, H)
    md = orc.expand_must_do_ref(list(md_tokens) if md_tokens else [0, 0], bn, kt + 1)
    p_round = {"bf16": True, "fp16": "f16", "e4m3": "fp8"}[dtype]
    out_dtype = torch.float16 if dtype == "fp16" else torch.bfloat16
    steps = []
    for step in range(STEPS):
        q, k, v = fragmented_qkv(B, Sq, Hk, D, seed=5, step=step, steps=STEPS, dtype=torch.float32, Sk=Sk)
        if H != Hk:
            q = gqa_heads(q, H // Hk)
        q, k, v = [_cast(dtype)(x) for x in (q, k, v)]
        rd, wr = lists[step % 2], lists[1 - step % 2]
        wr.zero_()
        margins = torch.empty(B, H, qt, kt)
        o, lse, n_tiles = orc.qkskip_fwd(q, k, v, block_m=bm, block_n=bn, read_list=rd, write_list=wr, must_do_list=md, thr=THR,
                                         margins=margins, p_round=p_round)
        assert n_tiles == orc.listed_tiles(rd)
        steps.append(dict(q=q, k=k, v=v, out=o.to(out_dtype), lse=lse, read=rd.clone(), write=wr.clone(), margins=margins))
    return dict(steps=steps, md=md, geom=(bm, bn, Sq, Sk, H, Hk, D, qt, kt), dtype=dtype, has_md=md_tokens is not None)


def _judge(run, st, out=None, lse=None, read=None):
    sc = _sc()
    bm, bn, Sq, Sk, H, Hk, D, qt, kt = run["geom"]
    return sc.sampled_row_check(st["q"], st["k"], st["v"], st["out"] if out is None else out, st["lse"] if lse is None else lse,
                                st["read"] if read is None else read, bm, bn, heads=range(H), n_rows=Sq + 8, **_bounds(run["dtype"]))     # + 8: sample_rows then takes every row


def _judge_lists(run, st, write=None, thr=THR, details=False):
    sc = _sc()
    bm, bn, Sq, Sk, H, Hk, D, qt, kt = run["geom"]
    items = list(itertools.product(range(H), range(qt)))
    return sc.vote_writer_check(st["q"], st["k"], st["read"], st["write"] if write is None else write, thr, bm, bn, items,
                                must_do_row=run["md"] if run["has_md"] else None, details=details)


@pytest.mark.parametrize("name", list(CASES))
def test_the_verdicts_accept_the_oracles_own_result(name):
    run = oracle_run(name)
    bm, bn, Sq, Sk, H, Hk, D, qt, kt = run["geom"]
    max_ranges, worst = 0, 0.0
    for i, st in enumerate(run["steps"]):
        res = _judge(run, st)
        print(f"{name} step {i}: sampled_row_check {res}")
        assert res["ok"] and res["rows"] == H * Sq, (i, res)
        vw = _judge_lists(run, st, details=True)
        print(f"{name} step {i}: vote_writer_check", {k_: v_ for k_, v_ in vw.items() if k_ != "details"})
        assert vw["ok"] and vw["items"] == H * qt and vw["bad"] == 0 and vw["borderline"] == 0 and vw["unexplained"] == 0 \
            and vw["unenumerated"] == 0, (i, vw)
        # the checker's margins are the oracle's, tile by tile (same walked tiles, same values up to fp32 summation order)
        for (h, m), d in vw["details"].items():
            mine, theirs = d["margin"], st["margins"][0, h, m]
            assert torch.equal(torch.isnan(mine), torch.isnan(theirs)), (h, m)
            if (~torch.isnan(mine)).any():
                worst = max(worst, (mine - theirs)[~torch.isnan(mine)].abs().max().item())
            assert d["status"] == "equal" and d["want"] == st["write"][0, h, m, : d["want"][0] + 1].tolist()
        max_ranges = max(max_ranges, int(st["read"][..., 0].max()) // 2, int(st["write"][..., 0].max()) // 2)
    print(f"{name}: max |checker margin - oracle margin| = {worst:.3e}, longest row {max_ranges} ranges")
    assert worst < 1e-3, worst
    assert max_ranges >= MIN_RANGES, f"longest row holds {max_ranges} ranges: the lists did not fragment"
    if run["has_md"]:
        sc = _sc()
        st = run["steps"][-1]
        flat_md = sc.lists_to_bitmap(st["write"])
        must = [n for n in range(kt) if any(e < n <= s for s, e in zip(run["md"].tolist()[1::2], run["md"].tolist()[2::2]))]
        assert len(must) >= 6 and bool(flat_md[..., must].all()), "a must-do tile the read list held was dropped"


# ---- d. mutations of O / LSE ---------------------------------------------------------------------------------------------------
def _ref(run, st, h, m, weights, hk=None):
    """fp32 attention of q-tile m of head h over keys weighted by ``weights`` (float [kt * bn]: 0 = tile not walked, 1 = walked, 2 =
    walked twice; K and V are zero padded behind seqlen_k, so a weight on a padding key is a key the seqlen mask failed to hide).
    Returns (O [rows, D], LSE [rows]). Walking a tile twice adds its keys twice to the row sums and to O."""
    bm, bn, Sq, Sk, H, Hk, D, qt, kt = run["geom"]
    hk = h // (H // Hk) if hk is None else hk
    pad = kt * bn - Sk
    qf = st["q"][0, m * bm: (m + 1) * bm, h].float()
    kf = torch.nn.functional.pad(st["k"][0, :, hk].float(), (0, 0, 0, pad))
    vf = torch.nn.functional.pad(st["v"][0, :, hk].float(), (0, 0, 0, pad))
    s = (qf @ kf.T) * D ** -0.5 + torch.log(weights)[None]
    return torch.softmax(s, dim=-1) @ vf, torch.logsumexp(s, dim=-1)


def _weights(run, row):
    bm, bn, Sq, Sk, H, Hk, D, qt, kt = run["geom"]
    w = torch.zeros(kt)
    w[_orc().walk_tiles(row)] = 1.0
    w = w.repeat_interleave(bn)
    w[Sk:] = 0.0
    return w


def _moved(run, true, mut):
    """How far a mutation moves the judged quantities, in units of the bound in force (the larger of the two), from two fp32 references."""
    b = _bounds(run["dtype"])
    o_bound = b["o_rtol"] * true[0].abs().max().item() + b["o_atol"]
    return max((mut[0] - true[0]).abs().max().item() / o_bound, (mut[1] - true[1]).abs().max().item() / b["lse_atol"])


def _planted(run, st, h, m, mut):
    """A copy of the oracle's O / LSE with q-tile m of head h replaced by a mutated reference (rounded as the output is)."""
    bm = run["geom"][0]
    out, lse = st["out"].clone(), st["lse"].clone()
    out[0, m * bm: (m + 1) * bm, h] = mut[0].to(out.dtype)
    lse[0, h, m * bm: (m + 1) * bm] = mut[1]
    return out, lse


def _reject(run, st, h, m, true, mut, what):
    factor = _moved(run, true, mut)
    print(f"{what}: head {h} q-tile {m} moves the judged quantity by {factor:.1f} x its bound")
    assert factor >= 10.0, f"{what}: the mutation moves the judged quantity by only {factor:.2f} x the bound; it proves nothing here"
    twin = _judge(run, st)
    assert twin["ok"], twin
    out, lse = _planted(run, st, h, m, mut)
    res = _judge(run, st, out=out, lse=lse)
    assert not res["ok"], (what, res)


def _best(run, st, candidates):
    """Among (h, m, weights-or-hk) candidates the one whose reference moves furthest from the true one."""
    best = None
    for h, m, kw in candidates:
        true = _ref(run, st, h, m, _weights(run, st["read"][0, h, m].tolist()))
        mut = _ref(run, st, h, m, **kw)
        f = _moved(run, true, mut)
        if best is None or f > best[0]:
            best = (f, h, m, true, mut)
    return best[1:]


@pytest.mark.parametrize("kind", ["tile-left-out", "unlisted-tile-walked", "tile-walked-twice"])
def test_sampled_row_check_rejects_a_wrong_walk(kind):
    run = oracle_run("bf16-256")
    st = run["steps"][-1]
    bm, bn, Sq, Sk, H, Hk, D, qt, kt = run["geom"]
    cands = []
    for h in range(H):
        for m in range(qt):
            row = st["read"][0, h, m].tolist()
            walk = _orc().walk_tiles(row)
            tiles = [t for t in range(kt - 1) if t not in walk] if kind == "unlisted-tile-walked" else walk[1:]   # never the first walked tile
            for t in tiles:
                w = _weights(run, row)
                w[t * bn: (t + 1) * bn] = {"tile-left-out": 0.0, "unlisted-tile-walked": 1.0, "tile-walked-twice": 2.0}[kind]
                cands.append((h, m, dict(weights=w)))
    assert cands
    h, m, true, mut = _best(run, st, cands)
    _reject(run, st, h, m, true, mut, kind)


def test_sampled_row_check_rejects_another_q_tiles_list():
    run = oracle_run("bf16-256")
    st = run["steps"][-1]
    qt = run["geom"][7]
    cands = [(h, m, dict(weights=_weights(run, st["read"][0, h, m2].tolist())))
             for h in range(run["geom"][4]) for m in range(qt) for m2 in ((m + 1) % qt,)
             if st["read"][0, h, m].tolist() != st["read"][0, h, m2].tolist()]
    assert cands, "every q-tile of a head reads the same list"
    h, m, true, mut = _best(run, st, cands)
    _reject(run, st, h, m, true, mut, "neighbour q-tile's list applied")


def test_sampled_row_check_rejects_gqa_heads_mapped_modulo():
    run = oracle_run("gqa-4-2")
    st = run["steps"][-1]
    bm, bn, Sq, Sk, H, Hk, D, qt, kt = run["geom"]
    cands = [(h, m, dict(weights=_weights(run, st["read"][0, h, m].tolist()), hk=h % Hk))
             for h in range(H) if h % Hk != h // (H // Hk) for m in range(qt)]
    assert cands
    h, m, true, mut = _best(run, st, cands)
    _reject(run, st, h, m, true, mut, "K/V head h % Hk")


def test_sampled_row_check_rejects_lse_in_base_2():
    run = oracle_run("bf16-256")
    st = run["steps"][-1]
    b = _bounds(run["dtype"])
    twin = _judge(run, st)
    assert twin["ok"], twin
    true = _ref(run, st, 0, 0, _weights(run, st["read"][0, 0, 0].tolist()))[1]
    moved = (true / LN2 - true).abs().max().item()
    assert moved >= 10 * b["lse_atol"], moved
    res = _judge(run, st, lse=st["lse"] / LN2)
    assert not res["ok"], res


def test_sampled_row_check_rejects_two_swapped_rows_of_the_short_last_q_tile():
    run = oracle_run("short-last-q-tile")
    st = run["steps"][-1]
    bm, bn, Sq, Sk, H, Hk, D, qt, kt = run["geom"]
    m = qt - 1
    n_last = Sq - m * bm
    assert 1 < n_last < bm
    best = None
    for h in range(H):
        true = _ref(run, st, h, m, _weights(run, st["read"][0, h, m].tolist()))
        for r in range(n_last - 1):                                                  # rows r, r + 1 of the last q-tile swapped
            perm = list(range(n_last))                                               # the reference holds the tile's real rows only
            perm[r], perm[r + 1] = perm[r + 1], perm[r]
            f = _moved(run, true, (true[0][perm], true[1][perm]))
            if best is None or f > best[0]:
                best = (f, h, r)
    f, h, r = best
    print(f"swapped rows {m * bm + r}, {m * bm + r + 1} of head {h}: {f:.1f} x the bound")
    assert f >= 10.0, f
    twin = _judge(run, st)
    assert twin["ok"], twin
    out, lse = st["out"].clone(), st["lse"].clone()
    a = m * bm + r
    out[0, [a, a + 1], h] = st["out"][0, [a + 1, a], h]
    lse[0, h, [a, a + 1]] = st["lse"][0, h, [a + 1, a]]
    res = _judge(run, st, out=out, lse=lse)
    assert not res["ok"], res


def test_sampled_row_check_rejects_unmasked_keys_behind_seqlen_k():
    """Flat rows (randn, scores of order 1), Sk = 2 tiles - 61 keys: the 61 zero keys behind seqlen_k would carry weight exp(0) each
    against a row sum of about 110. (On the fragmenting generator a row's sum is ~1e6 and the same fault hides below the bound, so
    that generator is not used here.)"""
    orc, sc = _orc(), _sc()
    B, Sq, Sk, H, D, bm, bn = 1, 300, 67, 2, 128, 256, 64
    qt, kt = -(-Sq // bm), -(-Sk // bn)
    g = torch.Generator().manual_seed(11)
    q, k, v = [torch.randn(B, n, H, D, generator=g).bfloat16() for n in (Sq, Sk, Sk)]
    lists = orc.init_skip_list_ref(B, qt, kt, H)
    o, lse, _ = orc.qkskip_fwd(q, k, v, block_m=bm, block_n=bn, read_list=lists[0], write_list=lists[1], thr=float("-inf"), p_round=True)
    st = dict(q=q, k=k, v=v, out=o.bfloat16(), lse=lse, read=lists[0])
    run = dict(geom=(bm, bn, Sq, Sk, H, H, D, qt, kt), dtype="bf16")
    h, m = 1, qt - 1
    w = _weights(run, lists[0][0, h, m].tolist())
    true = _ref(run, st, h, m, w)
    w_bad = w.clone()
    w_bad[Sk:] = 1.0
    mut = _ref(run, st, h, m, w_bad)
    assert true[0].shape[0] == Sq - m * bm                              # the ragged last q-tile as well
    _reject(run, st, h, m, true, mut, "keys behind seqlen_k unmasked")


# ---- d. mutations of the write list ------------------------------------------------------------------------------------------------
def _far_items(run, st, gap):
    """(h, m) whose walked tiles all vote at least ``gap`` away from the threshold by the ORACLE's margins: no borderline excuse."""
    H, qt = run["geom"][4], run["geom"][7]
    out = []
    for h in range(H):
        for m in range(qt):
            mg = st["margins"][0, h, m]
            mg = mg[~torch.isnan(mg)]
            if mg.numel() and bool(((mg - THR).abs() >= gap).all()):
                out.append((h, m))
    return out


def _put(st, h, m, row):
    wr = st["write"].clone()
    wr[0, h, m] = 0
    wr[0, h, m, : len(row)] = torch.tensor(row, dtype=torch.int32)
    return wr


def _flags_of(st, h, m):
    walk = _orc().walk_tiles(st["read"][0, h, m].tolist())
    return walk, [False] + [bool(st["margins"][0, h, m, t] <= THR) for t in walk[1:]]


@pytest.mark.parametrize("kind", ["vote-flipped", "L-plus-2", "L-minus-2", "entry-off-by-one", "neighbour-row", "first-tile-skipped"])
def test_vote_writer_check_rejects_a_wrong_row(kind):
    orc = _orc()
    run = oracle_run("bf16-256")
    st = run["steps"][-1]
    kt = run["geom"][8]
    twin = _judge_lists(run, st)
    assert twin["ok"] and twin["borderline"] == 0 and twin["unexplained"] == 0, twin
    done = False
    for h, m in _far_items(run, st, 0.1):                  # every vote of the row is at least 0.1 from thr: also the flipped one
        good = st["write"][0, h, m].tolist()
        L = good[0]
        good = good[: L + 1]
        walk, flags = _flags_of(st, h, m)
        assert orc.simulate_writer(st["read"][0, h, m].tolist(), flags) == good
        if kind == "vote-flipped":
            row = None
            for pos in range(1, len(walk)):
                f2 = list(flags)
                f2[pos] = not f2[pos]
                cand = orc.simulate_writer(st["read"][0, h, m].tolist(), f2)
                if cand != good:
                    row = cand
                    break
        elif kind == "L-plus-2":
            row = [L + 2] + good[1:] + [0, 0]
        elif kind == "L-minus-2":
            row = [L - 2] + good[1:] if L >= 4 else None
        elif kind == "entry-off-by-one":
            row = good[: L] + [good[L] + 1] if L >= 2 else None
        elif kind == "neighbour-row":
            other = st["write"][0, h, (m + 1) % run["geom"][7]].tolist()
            row = other[: other[0] + 1]
        else:                                              # the first walked tile recorded as skipped: the row opens one tile further down
            row = ([L, kt - 2] + good[2:]) if good[2] < kt - 1 else ([L - 2] + good[3:] if L >= 4 else None)
        if row is None or row == good or len(row) > kt + 1:
            continue
        res = _judge_lists(run, st, write=_put(st, h, m, row))
        assert not res["ok"] and res["bad"] == 1, (kind, h, m, good, row, res)
        done = True
        break
    assert done, f"no item to plant '{kind}' on"


def test_vote_writer_check_rejects_a_dropped_must_do_tile():
    orc = _orc()
    run = oracle_run("must-do")
    assert run["has_md"] and run["md"][0] >= 6                   # a multi-range must-do row
    planted = 0
    for st in run["steps"]:
        twin = _judge_lists(run, st)
        assert twin["ok"] and twin["borderline"] == 0 and twin["unexplained"] == 0, twin
        for h, m in _far_items(run, st, 0.1):
            walk, flags = _flags_of(st, h, m)
            rd = st["read"][0, h, m].tolist()
            good = orc.simulate_writer(rd, flags, run["md"].tolist())
            assert good == st["write"][0, h, m, : good[0] + 1].tolist()
            row = orc.simulate_writer(rd, flags)                  # the writer without its must-do list
            if row == good:
                continue
            assert set(orc.walk_tiles(row)) < set(orc.walk_tiles(good))       # what it drops is must-do tiles
            res = _judge_lists(run, st, write=_put(st, h, m, row))
            assert not res["ok"] and res["bad"] == 1, (h, m, good, row, res)
            # and a checker that is not told about the must-do list rejects the TRUE row
            sc = _sc()
            bm, bn = run["geom"][:2]
            blind = sc.vote_writer_check(st["q"], st["k"], st["read"], st["write"], THR, bm, bn, [(h, m)])
            assert not blind["ok"]
            planted += 1
            break
    assert planted >= 1, "the must-do list never changed a written row"


def test_a_close_vote_excuses_only_what_its_flip_reproduces():
    """thr is placed 5e-4 above one tile's margin, so that vote is close. The row written with that vote flipped is borderline and
    explained; the same row with an unrelated entry off by one is borderline (a close vote exists) but unexplained."""
    orc, sc = _orc(), _sc()
    run = oracle_run("bf16-256")
    st = run["steps"][-1]
    bm, bn, Sq, Sk, H, Hk, D, qt, kt = run["geom"]
    checked = 0
    for h, m in itertools.product(range(H), range(qt)):
        rd = st["read"][0, h, m].tolist()
        walk = orc.walk_tiles(rd)
        mg = st["margins"][0, h, m]
        for pos in range(1, len(walk)):
            thr = float(mg[walk[pos]]) + 5e-4
            others = torch.tensor([float(mg[t]) for i, t in enumerate(walk) if i not in (0, pos)])
            if others.numel() < 2 or bool(((others - thr).abs() < 0.01).any()):
                continue
            flags = [False] + [bool(mg[t] <= thr) for t in walk[1:]]
            good = orc.simulate_writer(rd, flags)
            f2 = list(flags)
            f2[pos] = not f2[pos]
            flipped = orc.simulate_writer(rd, f2)
            if flipped == good or flipped[0] < 2 or flipped[-1] == kt - 1:
                continue
            kw = dict(thr=thr, block_m=bm, block_n=bn, items=[(h, m)])
            r0 = sc.vote_writer_check(st["q"], st["k"], st["read"], _put(st, h, m, good), **kw)
            assert (r0["bad"], r0["borderline"], r0["unexplained"]) == (0, 0, 0), r0
            r1 = sc.vote_writer_check(st["q"], st["k"], st["read"], _put(st, h, m, flipped), details=True, **kw)
            assert (r1["bad"], r1["borderline"], r1["unexplained"], r1["unenumerated"]) == (0, 1, 0, 0) and r1["ok"], r1
            assert r1["details"][(h, m)]["status"] == "explained"
            broken = flipped[:-1] + [flipped[-1] + 1]
            r2 = sc.vote_writer_check(st["q"], st["k"], st["read"], _put(st, h, m, broken), details=True, **kw)
            assert (r2["bad"], r2["borderline"], r2["unexplained"]) == (0, 1, 1), r2
            assert r2["details"][(h, m)]["status"] == "unexplained"
            checked += 1
            break
        if checked >= 3:
            break
    assert checked >= 3


def test_rows_with_many_close_votes_are_counted_apart(monkeypatch):
    sc = _sc()
    run = oracle_run("bf16-256")
    st = run["steps"][-1]
    h, m = 0, 0
    monkeypatch.setattr(sc, "EXPLAIN_MAX_CLOSE", 0)
    good = st["write"][0, h, m].tolist()
    broken = _put(st, h, m, good[: good[0]] + [good[good[0]] + 1])
    bm, bn = run["geom"][:2]
    res = sc.vote_writer_check(st["q"], st["k"], st["read"], broken, THR, bm, bn, [(h, m)], margin_tol=100.0)     # every vote "close"
    assert (res["bad"], res["borderline"], res["unenumerated"], res["unexplained"]) == (0, 1, 1, 0) and res["ok"], res
