"""GPU: the three multi-GPU drivers of liteattention_amd.parallel on the REAL kernels, worlds of 2 and 3 in one process on one
device (tests/lockstep_ranks.py: every rank a thread with its own driver object, the collectives plain device copies; pinned against
gloo by tests/test_lockstep_ranks_cpu.py). What runs here and nowhere else: Ulysses' reshapes around a kernel that writes lists by
local head, the ring's choice of skip state and of the descales that travel with a K/V shard, the merge of the ring's stacked
partials, the overlapped all-gather's non-contiguous row windows at B > 1, the slicing of a head-threshold table.

Every driver is compared bit for bit (O and skip lists, three calls in a row: the lists ping-pong) with the single-rank product path
- one LiteAttention over all heads; for the ring one SeqParallelLiteAttention driven by hand - and O, through that equality, with a
CPU reference under the reference project's tolerance rule. Inputs, references, rule and the checks that the references can tell
the mistakes apart: tests/parallel_rank_cases.py. RCCL itself is not here: tests/test_gpu_rccl_world1.py and an N-GPU node."""
import pytest
import torch

import lockstep_ranks as ls
import parallel_rank_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda"
TIMEOUT_S = 60.0


def _L():
    import liteattention_amd as L
    return L


def _run(world, fn):
    with ls.distributed() as group:
        res = ls.run_ranks(world, lambda rank: fn(rank, group), timeout_s=TIMEOUT_S)
    torch.cuda.synchronize()
    return res


def _within(name, out, o_ref, tol):
    err = (out.double().cpu() - o_ref.double()).abs().max().item()
    print(f"  {name}: max|O - reference| = {err:.4g}, tolerance {tol:.4g}")
    assert err <= tol, (name, err, tol)


def _lists_are_the_oracles(name, lists, oracle_rows):
    """The product's lists against the chained oracle's, on what a reader walks of each row ([length, entries...]; the kernel leaves
    what lies behind untouched). This makes the input conditions, which are statements about the oracle, statements about the kernel."""
    mine = lists.cpu().to(torch.int32)
    assert mine.shape == oracle_rows.shape, (name, mine.shape, oracle_rows.shape)
    for a, e in zip(mine.reshape(-1, mine.shape[-1]), oracle_rows.reshape(-1, mine.shape[-1])):
        n = int(e[0])
        assert torch.equal(a[: n + 1], e[: n + 1]), (name, a.tolist(), e.tolist())


def _full_path(case):
    """One LiteAttention over all heads, three calls: per step (O, both lists)."""
    L = _L()
    q, k, v = [x.to(case["dtype"]).to(DEV) for x in (case["q"], case["k"], case["v"])]
    full = L.LiteAttention(enable_skipping=not case["dense"], threshold=pc.THR, max_batch_size=pc.B)
    if case["table"] is not None:
        full.set_head_thresholds(case["table"])
    steps = []
    for _ in range(pc.STEPS):
        out = full(q, k, v)
        steps.append((out.clone(), None if case["dense"] else full._skip_list.clone()))
    return (q, k, v), steps


# ------------------------------------------------------------------------------------------------------------------- head-sharded
@pytest.mark.parametrize("table", [False, True], ids=["scalar_thr", "head_table"])
@pytest.mark.parametrize("overlap", [False, True], ids=["plain", "overlapped"])
@pytest.mark.parametrize("world", [2, 3])
def test_head_sharded_ranks_equal_one_lite_attention_over_all_heads(world, overlap, table):
    """G ranks, each on its heads, plain all-gather or three overlapped row windows (uneven, the last one the partial q-tile; B = 2, so
    no window's rows are one slab): every rank's gathered result is the single LiteAttention's, bit for bit, at each of three steps;
    rank r's lists are that object's lists of heads [h0, h1); with a table of 6 distinct head thresholds the same."""
    from liteattention_amd.parallel import HeadShardedLiteAttention
    case = pc.full_case(world, "bf16", table, False)
    pc.check_full_case(case)
    (q, k, v), full = _full_path(case)
    windows = pc.q_windows(case["S"], case["bm"])
    rows = [min(case["S"], (t0 + n) * case["bm"]) - t0 * case["bm"] for t0, n in windows]
    Hl = pc.H // world

    def rank_fn(rank, group):
        att = HeadShardedLiteAttention(num_heads=pc.H, threshold=pc.THR, max_batch_size=pc.B, process_group=group,
                                       overlap_windows=3 if overlap else 1)
        assert (att.world, att.rank, att.h0, att.h1) == (world, rank, rank * Hl, (rank + 1) * Hl)
        if overlap:
            att.q_windows = lambda q_: windows
        if table:
            att.set_head_thresholds(case["table"])
        steps = []
        for _ in range(pc.STEPS):
            res = att(att.shard(q), att.shard(k), att.shard(v))
            if overlap:
                assert [tuple(b.shape) for b in res] == [(world, pc.B, n, Hl, case["D"]) for n in rows]
            else:
                assert tuple(res.shape) == (world, pc.B, case["S"], Hl, case["D"])
            steps.append((HeadShardedLiteAttention.to_bshd(res).clone(), att.local._skip_list.clone()))
        return steps

    ranks = _run(world, rank_fn)
    for step, (o_full, lists_full) in enumerate(full):
        for r in range(world):
            o_r, lists_r = ranks[r][step]
            assert torch.equal(o_r, o_full), f"step {step}: rank {r}'s gathered output is not the single LiteAttention's"
            assert torch.equal(o_r, ranks[0][step][0]), f"step {step}: ranks 0 and {r} hold different gathered bits"
            assert lists_r.shape[1] == pc.B and torch.equal(lists_r, lists_full[:, :, r * Hl:(r + 1) * Hl]), \
                f"step {step}: rank {r}'s skip lists are not those of heads [{r * Hl}, {(r + 1) * Hl})"
        _within(f"step {step}", o_full, case["o_ref"][step], case["tol"][step])
    _lists_are_the_oracles("written at the last step", full[-1][1][pc.STEPS % 2], case["written"][-1])


# ------------------------------------------------------------------------------------------------------------------------ Ulysses
@pytest.mark.parametrize("kind,table", [("bf16", False), ("bf16", True), ("fp16", False)], ids=["bf16_d128", "bf16_d128_head_table", "fp16_d64"])
@pytest.mark.parametrize("world", [2, 3])
def test_ulysses_ranks_equal_one_lite_attention_on_the_full_sequence(world, kind, table):
    """Rows in, rows out, heads inside: the ranks' outputs concatenated over rows are the single LiteAttention's bits on the full
    sequence (whose q-tiles cut across the former rank boundaries), rank r's lists are its lists of heads [h0, h1), O is the
    reference's under the rule; three steps."""
    from liteattention_amd.parallel import UlyssesLiteAttention
    case = pc.full_case(world, kind, table, False)
    pc.check_full_case(case)
    (q, k, v), full = _full_path(case)
    Hl = pc.H // world

    def rank_fn(rank, group):
        uly = UlyssesLiteAttention(num_heads=pc.H, threshold=pc.THR, max_batch_size=pc.B, process_group=group)
        if table:
            uly.set_head_thresholds(case["table"])
        mine = [x[:, rank * pc.SL:(rank + 1) * pc.SL].contiguous() for x in (q, k, v)]
        steps = []
        for _ in range(pc.STEPS):
            out = uly(*mine)
            assert tuple(out.shape) == (pc.B, pc.SL, pc.H, case["D"]) and out.dtype == case["dtype"]
            steps.append((out.clone(), uly.local._skip_list.clone()))
        return steps

    ranks = _run(world, rank_fn)
    for step, (o_full, lists_full) in enumerate(full):
        rows = torch.cat([ranks[r][step][0] for r in range(world)], dim=1)
        assert torch.equal(rows, o_full), f"step {step}: the ranks' rows are not the single LiteAttention's output"
        for r in range(world):
            assert torch.equal(ranks[r][step][1], lists_full[:, :, r * Hl:(r + 1) * Hl]), f"step {step}: rank {r}'s skip lists"
        _within(f"step {step}", rows, case["o_ref"][step], case["tol"][step])
    _lists_are_the_oracles("written at the last step", full[-1][1][pc.STEPS % 2], case["written"][-1])


@pytest.mark.parametrize("world", [2, 3])
def test_ulysses_without_skipping_is_dense_attention(world):
    from liteattention_amd.parallel import UlyssesLiteAttention
    case = pc.full_case(world, "bf16", False, True)
    pc.check_full_case(case)
    q, k, v = [x.to(case["dtype"]).to(DEV) for x in (case["q"], case["k"], case["v"])]

    def rank_fn(rank, group):
        uly = UlyssesLiteAttention(num_heads=pc.H, enable_skipping=False, max_batch_size=pc.B, process_group=group)
        out = uly(*[x[:, rank * pc.SL:(rank + 1) * pc.SL].contiguous() for x in (q, k, v)])
        assert uly.local._skip_list is None
        return out

    _within("dense", torch.cat(_run(world, rank_fn), dim=1), case["o_ref"][0], case["tol"][0])


# --------------------------------------------------------------------------------------------------------------------------- ring
def _ring_inputs(case):
    dev = lambda xs: [x.to(case["dtype"]).to(DEV) for x in xs]               # noqa: E731
    q, k, v = dev(case["q"]), dev(case["k"]), dev(case["v"])
    if case["descales"] is None:
        return q, k, v, (lambda r, j: {})
    qd, kd, vd = [[d.to(DEV) for d in ds] for ds in case["descales"]]
    return q, k, v, (lambda r, j: dict(q_descale=qd[r], k_descale=kd[j], v_descale=vd[j]))


_RING_RUNS = {}


def _ring_run(kw):
    """One ring case on the device, once for the tests that read it: (case, hand, ranks). hand[r][step] = (O, LSE, lists of every
    state) of one SeqParallelLiteAttention per rank driven by hand - shard j on state j, partials stacked in the ring's order r, r-1, ...
    and merged by flash_attn_combine; ranks[r][step] = (O, lists of every state) of the driver under the lockstep harness."""
    key = pc.case_id(kw)
    if key not in _RING_RUNS:
        try:
            _RING_RUNS[key] = _ring_run_once(kw)
        except BaseException as exc:          # a case that failed is not run on the device a second time: its other test gets the same error
            _RING_RUNS[key] = exc
    if isinstance(_RING_RUNS[key], BaseException):
        raise _RING_RUNS[key]
    return _RING_RUNS[key]


def _ring_run_once(kw):
    L = _L()
    from liteattention_amd.parallel import RingSeqParallelLiteAttention
    case = pc.ring_case(**kw)
    pc.check_ring_case(case)
    G, batch, dense = case["world"], case["batch"], case["dense"]
    q, k, v, descales = _ring_inputs(case)
    # 16-bit partials that are merged run with the exact rescale (RingSeqParallelLiteAttention._partial says why): the hand-driven path asks
    # for it by the public scope; the lists do not depend on it (tests/test_gpu_round2.py). That the ring NEEDS it is not shown by this
    # equality but by test_ring_output_against_the_fp64_merge_of_the_oracle_partials, whose reference knows no flag
    exact = L._cabi.LA_FLAG_EXACT_RESCALE if case["descales"] is None else 0
    hand = []
    for r in range(G):
        sp = L.SeqParallelLiteAttention(G, enable_skipping=not dense, threshold=pc.THR, max_batch_size=batch)
        if case["table"] is not None:
            sp.set_head_thresholds(case["table"])
        steps = []
        for _ in range(pc.STEPS):
            with L.flash_attn_interface.fwd_flags(exact):
                parts = [sp(q[r], k[j], v[j], j, return_softmax_lse=True, **descales(r, j)) for j in pc.ring_order(G, r)]
            out, lse = L.flash_attn_combine(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
            assert tuple(lse.shape) == (batch, case["heads"], case["sl"])
            steps.append((out.clone(), lse.clone(), None if dense else [la._skip_list.clone() for la in sp.lite_attention]))
        hand.append(steps)

    def rank_fn(rank, group):
        ring = RingSeqParallelLiteAttention(enable_skipping=not dense, threshold=pc.THR, max_batch_size=batch, process_group=group)
        assert (ring.world, ring.rank) == (G, rank)
        if case["table"] is not None:
            ring.set_head_thresholds(case["table"])
        steps = []
        for _ in range(pc.STEPS):
            out = ring(q[rank], k[rank], v[rank], **descales(rank, rank))
            assert tuple(out.shape) == (batch, case["sl"], case["heads"], case["D"]) and out.dtype == case["out_dtype"]
            steps.append((out.clone(), None if dense else [la._skip_list.clone() for la in ring.states.lite_attention]))
        return steps

    return case, hand, _run(G, rank_fn)


@pytest.mark.parametrize("kw", pc.RING_CASES, ids=pc.case_id)
def test_ring_ranks_equal_the_hand_driven_single_rank_path(kw):
    """Rank r keeps its query rows, the K/V shards (e4m3: with their own k / v descales; q's differs per rank) come round the ring.
    Against the hand-driven single-rank path (``_ring_run``): the same output bits, the same lists in EVERY state j, at each of three
    steps; the lists written last are the chained oracle's; bf16 / fp16: the merged LSE within 1e-3 of the fp64 merge's (the bound of
    test_seq_parallel_splits_plus_combine_equal_full_attention). Cases: worlds 2 and 3 in bf16, fp16, e4m3; a head-threshold table;
    B = 1; and Sl == H == 8, dense, where flash_attn_combine has only the strides to tell the two LSE layouts apart."""
    case, hand, ranks = _ring_run(kw)
    G, dense = case["world"], case["dense"]
    for r in range(G):
        for step in range(pc.STEPS):
            o_hand, lse_hand, lists_hand = hand[r][step]
            o_ring, lists_ring = ranks[r][step]
            assert torch.equal(o_ring, o_hand), f"rank {r}, step {step}: the ring's output is not the hand-driven path's"
            if not dense:
                for j in range(G):
                    assert lists_ring[j].shape[1] == case["batch"]
                    assert torch.equal(lists_ring[j], lists_hand[j]), f"rank {r}, step {step}: state {j} holds other lists"
                if step == pc.STEPS - 1:
                    for j in range(G):
                        _lists_are_the_oracles(f"rank {r}, state {j}", lists_hand[j][pc.STEPS % 2], case["ranks"][r][1][j][-1][3])
            if case["descales"] is None:
                lse_err = (lse_hand.double().cpu() - case["ranks"][r][0][step][2]).abs().max().item()
                print(f"  rank {r}, step {step}: max|LSE - reference| = {lse_err:.4g}")
                assert lse_err <= 1e-3, (r, step, lse_err)


@pytest.mark.parametrize("kw", pc.RING_CASES, ids=pc.case_id)
def test_ring_output_against_the_fp64_merge_of_the_oracle_partials(kw):
    """O of every rank and step under the rule of tests/parallel_rank_cases.py: ``dense_tolerance(out_ref, out_pt)``, out_ref the fp64
    merge of the per-pair oracle results, out_pt the merge of those partials each rounded to the output type (e4m3: the fp8 bound).
    Every figure is printed before the one assertion.

    This test is what keeps the ring's exact rescale (``RingSeqParallelLiteAttention._partial``). With the forward's default, lazy
    rescale the world-3 cases miss the rule on the MI355X (max|O - reference| / tolerance; everything else passed, world 2 at 0.5-0.74):
      world3-kindbf16            rank 1: 0.008621 / 0.008484 (1.016) at step 0, 0.008486 / 0.008489 (1.000) at steps 1, 2
      world3-kindbf16-tableTrue  rank 1: 0.008621 / 0.008484 (1.016) at step 0, 0.008533 / 0.008489 (1.005) at steps 1, 2
      world3-kindfp16            rank 2: 0.001955 / 0.001623 (1.204) at step 0, 0.001896 / 0.001623 (1.168) at steps 1, 2
    Cause, from the partials of these two ranks taken apart on the CPU: LSE (2e-6), la_combine (the fp64 merge of the kernel's own
    partials before its one rounding) and the lists are right; what is larger than in the reference's arithmetic is the 16-bit rounding
    of P. Lazily, P = exp2((S - m_ref) c) with m_ref an OLDER row maximum, so the weight of the row's largest key is not exactly 1 and is
    rounded like any other; relative to the true running maximum it is exact. Common factor of a row of a partial, rms of (O / O_fp64
    - 1): kernel 7.9e-4 (bf16) / 1.1e-4 (fp16); a fp64 model with P rounded relative to the row maximum 3.4e-4 / 4.5e-5, relative to
    the first tile's maximum 7.1e-4, to the maximum + 0.3: 8.8e-4 / 8.7e-5. One launch stays inside the rule with that; three partials,
    each rounded once more before the merge, do not. The oracle with P in the 16-bit type (``qkskip_fwd(p_round=True / "f16")``,
    relative to the true maximum) sits at 0.50-0.52 of the tolerance in every world-3 case, and so does the ring with the exact
    rescale (0.50-0.52 in every bf16 / fp16 case; e4m3 0.20-0.34): the rule as the issue states it holds, nothing is widened."""
    case, _, ranks = _ring_run(kw)
    missed = []
    for r in range(case["world"]):
        for step in range(pc.STEPS):
            o_ref, tol = case["ranks"][r][0][step][0], case["tol"][r][step]
            err = (ranks[r][step][0].double().cpu() - o_ref).abs().max().item()
            print(f"  rank {r}, step {step}: max|O - reference| = {err:.4g}, tolerance {tol:.4g}, ratio {err / tol:.3f}")
            if not err <= tol:
                missed.append((r, step, err, tol))
    assert not missed, missed


def test_ring_exact_partials_is_the_difference_to_the_lazy_forward():
    """``exact_partials`` of the ring driver, world 3 in bf16, first call: switched off, every rank's output is the merge of the
    forward's DEFAULT (lazily rescaled) partials, bit for bit - the hand-driven path without any flag - and is not the default ring's
    output; the lists are the same either way. The lazy figures against the O rule are printed, not asserted: they are the miss
    (rank 1: 1.016) that test_ring_output_against_the_fp64_merge_of_the_oracle_partials records and the switch's default closes."""
    L = _L()
    from liteattention_amd.parallel import RingSeqParallelLiteAttention
    kw = dict(world=3, kind="bf16")
    case, _, exact = _ring_run(kw)
    G = case["world"]
    q, k, v, _ = _ring_inputs(case)
    hand = []
    for r in range(G):
        sp = L.SeqParallelLiteAttention(G, threshold=pc.THR, max_batch_size=pc.B)
        parts = [sp(q[r], k[j], v[j], j, return_softmax_lse=True) for j in pc.ring_order(G, r)]
        hand.append(L.flash_attn_combine(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))[0].clone())

    def rank_fn(rank, group):
        ring = RingSeqParallelLiteAttention(threshold=pc.THR, max_batch_size=pc.B, process_group=group)
        assert ring.exact_partials is True
        ring.exact_partials = False
        out = ring(q[rank], k[rank], v[rank])
        return out.clone(), [la._skip_list.clone() for la in ring.states.lite_attention]

    lazy = _run(G, rank_fn)
    for r in range(G):
        o_ref, tol = case["ranks"][r][0][0][0], case["tol"][r][0]
        err = (lazy[r][0].double().cpu() - o_ref).abs().max().item()
        print(f"  rank {r}, lazy partials: max|O - reference| = {err:.4g}, tolerance {tol:.4g}, ratio {err / tol:.3f}")
        assert torch.equal(lazy[r][0], hand[r]), f"rank {r}: exact_partials = False is not the merge of the forward's default partials"
        assert not torch.equal(lazy[r][0], exact[r][0][0]), f"rank {r}: the exact rescale changed nothing"
        for j in range(G):
            assert torch.equal(lazy[r][1][j], exact[r][0][1][j]), f"rank {r}, state {j}: the lists depend on exact_partials"
