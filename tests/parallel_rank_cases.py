"""Inputs, CPU references and input conditions of tests/test_gpu_parallel_ranks.py (no GPU needed; the conditions and sensitivity
margins are run against the oracle alone by tests/test_lockstep_ranks_cpu.py).

Shapes: B = 2, H = 6 (worlds of 2 and 3 divide it), Sl = 328 rows per rank - no multiple of the 64-key tile nor of the 128- / 256-row
q-tile, so the last q-tile of every shard is partial and the q-tiles of the full sequence S = G * Sl cut across former rank boundaries.

Inputs are of the structured form of ``helpers.structured_qkv`` (``alpha * direction of the row's frame + noise``), with two changes
these shapes need. (1) The frames draw their direction from a dictionary of 3 per (batch, head), so that the queries of one shard
find matching keys in EVERY K/V shard: with one direction per frame of the whole sequence, as ``structured_qkv`` has it, a (Q shard
r x K/V shard j != r) pair has no structure and drops nothing. (2) The key frames are 82 rows (4 per shard, cutting the 64-key tiles)
but a query frame is a whole shard: a tile is dropped only when EVERY row of the q-tile has met a far better key earlier in the walk,
the 256-row q-tile is most of a shard, and the partial last q-tile never drops anything (its zero rows vote 0). Heads, batches and
shards still differ from one another.

References. Dense: ``oracle.attention_dense_ref`` in fp64. With skipping: ``oracle.qkskip_fwd`` (fp32 accumulation, un-rounded P; for
e4m3 the reference's e4m3 P, the oracle of tests/test_gpu_round4.py) at the kernel's tile geometry, the lists chained over the steps
by the oracle alone. The ring: one such chain per (Q shard r, K/V shard j), merged by ``oracle.attention_combine_ref`` in fp64.

Rule for O: ``oracle.dense_tolerance(out_ref, out_pt)`` (the reference project's rule), ``out_pt`` = the reference rounded once to the
output type; for the ring ``out_pt`` = the merge of the partials each rounded to the output type, itself a tensor of the output type
(as every ``out_pt`` of the reference's rule is). e4m3: ``0.05 max|O_ref| + 2e-2``, the stated fp8 bound of tests/test_gpu_round4.py.
This is tighter than the rule as the reference project applies it, twice over: there ``out_pt`` is a whole forward in the 16-bit type
(scores and P rounded), here only the output roundings; and the rule's second term, ``2 max|out_ref + 0.3 - 0.3 - out_ref|``, is
taken there on an ``out_ref`` held in the output type (a few of its ulps) and is zero on the fp64 ``out_ref`` used here.

Conditions on the inputs (``check_*``; a seed that misses one is replaced, the assertion stays): at the last step every (rank, state)
reads a list that has dropped at least one tile and kept at least two; no vote of any step lies within 1e-3 of its threshold (the
borderline rule of tests/test_gpu_parity.py: fp32 summation order may flip such a tile, and the chained oracle would then walk other
tiles than the kernel); the lists hold exactly B sequences, so no compared list row is one that no call reads or writes.
Sensitivity (each margin is printed): exchanging two head blocks or two row shards of the reference, pairing a shard with another
shard's e4m3 descales, and rotating the head-threshold table by one head all move the reference by more than the tolerance / change
the lists, and the ring's lists of states j != j' differ for every rank - so equality with a path that shared such a mistake would
not go unnoticed."""
import functools

import torch

F8 = torch.float8_e4m3fn
B, H, SL, STEPS, THR = 2, 6, 328, 3, -3.0
FRAME, N_DIRS = 82, 3
# dtype, head dim, alpha, p_round of the skipping reference, seed
KINDS = {"bf16": (torch.bfloat16, 128, 10.0, False, 11), "fp16": (torch.float16, 64, 10.0, False, 12), "e4m3": (F8, 128, 10.0, "fp8", 13)}
HEAD_TABLE = [-3.0, -5.0, -6.0, -7.0, -8.0, -10.0]          # one threshold per head, all distinct
BORDERLINE = 1e-3


# every case tests/test_gpu_parallel_ranks.py runs: arguments of full_case / ring_case
FULL_CASES = [(w, kind, table, False) for w in (2, 3) for kind, table in (("bf16", False), ("bf16", True), ("fp16", False))] + \
             [(w, "bf16", False, True) for w in (2, 3)]
RING_CASES = [dict(world=w, kind=kind) for w in (2, 3) for kind in ("bf16", "fp16", "e4m3")] + \
             [dict(world=w, kind="bf16", table=True) for w in (2, 3)] + \
             [dict(world=2, kind="bf16", batch=1, reseed=1),      # the first seed left (rank 1, state 0) with nothing dropped
              dict(world=2, kind="bf16", heads=8, sl=8, dense=True)]    # Sl == H: flash_attn_combine must tell the LSE layouts apart by strides


def case_id(c):
    return "-".join(f"{k}{v}" for k, v in c.items()) if isinstance(c, dict) else f"world{c[0]}-{c[1]}" + "-table" * c[2] + "-dense" * c[3]


def _orc():
    from oracle import oracle as orc
    return orc


def tiles(kind):
    import liteattention_amd as L
    dtype, D = KINDS[kind][:2]
    return L.get_tile_sizes(D, dtype.itemsize)


def structured_shards(S, D, alpha, seed, batch=B, heads=H, dtype=torch.bfloat16, sl=SL):
    """(q, k, v) of shape (batch, S, heads, D) on the CPU, fp32 values representable in ``dtype`` (module docstring)."""
    g = torch.Generator().manual_seed(seed)
    dirs = torch.randn(batch, N_DIRS, heads, D, generator=g)
    dirs = dirs / dirs.norm(dim=-1, keepdim=True)
    which_q = torch.randint(0, N_DIRS, (batch, -(-S // sl), heads), generator=g)
    which_k = torch.randint(0, N_DIRS, (batch, -(-S // FRAME), heads), generator=g)
    pick = lambda which, per: dirs.gather(1, which[:, torch.arange(S) // per][..., None].expand(batch, S, heads, D))   # noqa: E731
    q = alpha * pick(which_q, sl) + torch.randn(batch, S, heads, D, generator=g)
    k = alpha * pick(which_k, FRAME) + torch.randn(batch, S, heads, D, generator=g)
    v = torch.randn(batch, S, heads, D, generator=g)
    return [x.to(dtype).float() for x in (q, k, v)]


def shard_descales(world, seed, batch=B, heads=H):
    """e4m3: (q_descale per rank, k_descale per shard, v_descale per shard), each fp32 (batch, heads), far apart between shards."""
    g = torch.Generator().manual_seed(seed)
    base_q, base_k, base_v = [0.9, 1.1, 1.0], [1.3, 1.0, 0.75], [0.6, 1.0, 1.4]
    mk = lambda base: [base[i] + 0.1 * torch.rand(batch, heads, generator=g) for i in range(world)]      # noqa: E731
    return mk(base_q), mk(base_k), mk(base_v)


def q_windows(S, bm):
    """Three uneven windows of q-tiles, the last one ending in the partial q-tile."""
    qt = -(-S // bm)
    assert qt >= 3 and S % bm != 0
    return [(0, 1), (1, qt - 2), (qt - 1, 1)]


def listed(row_lists):
    """(listed tiles, all tiles) of lists [..., Qt, Kt + 1]."""
    orc = _orc()
    flat = row_lists.reshape(-1, row_lists.shape[-1])
    return orc.listed_tiles(flat), flat.shape[0] * (flat.shape[1] - 1)


def oracle_chain(q, k, v, bm, bn, p_round, steps=STEPS, thr=THR, head_thr=None, descales=None, dense=False):
    """``steps`` calls of one LiteAttention, by the oracle alone: [(o fp32 (B,Sq,H,D), lse (B,H,Sq), list read, list written)] and the
    smallest |vote - threshold| of all steps. ``head_thr``: one threshold per head (the oracle takes a scalar: one head at a time)."""
    orc = _orc()
    Bq, Sq, Hq, _ = q.shape
    Qt, Kt = -(-Sq // bm), -(-k.shape[1] // bn)
    kw = {} if descales is None else dict(zip(("q_descale", "k_descale", "v_descale"), descales))
    if dense:
        o, lse, _ = orc.qkskip_fwd(q, k, v, block_m=bm, block_n=bn, p_round=p_round, **kw)
        return [(o, lse, None, None)] * steps, float("inf")
    lists = orc.init_skip_list_ref(Bq, Qt, Kt, Hq)
    md_row = orc.expand_must_do_ref([0, 0], bn, Kt + 1)
    out, closest = [], float("inf")
    for step in range(steps):
        rd, wr = lists[step % 2].clone(), torch.zeros_like(lists[0])        # (a copy: the next step but one writes this slot again)
        margins = torch.empty(Bq, Hq, Qt, Kt)
        if head_thr is None:
            o, lse, _ = orc.qkskip_fwd(q, k, v, block_m=bm, block_n=bn, read_list=rd, write_list=wr, must_do_list=md_row, thr=thr,
                                       p_round=p_round, margins=margins, **kw)
            dist_thr = (margins - thr).abs()
        else:
            o, lse = torch.empty(Bq, Sq, Hq, v.shape[3]), torch.empty(Bq, Hq, Sq)
            for h in range(Hq):
                hs = slice(h, h + 1)
                wr_h, mg_h = torch.zeros_like(wr[:, hs]), torch.empty(Bq, 1, Qt, Kt)
                kw_h = {name: d[:, hs] for name, d in kw.items()}
                o[:, :, hs], lse[:, hs], _ = orc.qkskip_fwd(q[:, :, hs], k[:, :, hs], v[:, :, hs], block_m=bm, block_n=bn,
                                                           read_list=rd[:, hs].contiguous(), write_list=wr_h, must_do_list=md_row,
                                                           thr=float(head_thr[h]), p_round=p_round, margins=mg_h, **kw_h)
                wr[:, hs], margins[:, hs] = wr_h, mg_h
            dist_thr = (margins - torch.tensor(head_thr).view(1, Hq, 1, 1)).abs()
        dist_thr = dist_thr[~torch.isnan(dist_thr)]
        if dist_thr.numel():
            closest = min(closest, dist_thr.min().item())
        lists[1 - step % 2] = wr
        out.append((o, lse, rd, wr.clone()))
    return out, closest


def o_tolerance(kind, out_ref, out_pt=None):
    orc = _orc()
    dtype = KINDS[kind][0]
    if dtype == F8:
        return 0.05 * out_ref.abs().max().item() + 2e-2
    if out_pt is None:
        out_pt = out_ref.to(dtype)
    return orc.dense_tolerance(out_ref, out_pt)


# ----------------------------------------------------------------------------------------- head-sharded and Ulysses: the full sequence
@functools.lru_cache(maxsize=None)
def full_case(world, kind, table=False, dense=False):
    """One LiteAttention over all heads of the full (B, world * SL, H, D) tensors: inputs, per-step references and tolerances."""
    orc = _orc()
    dtype, D, alpha, p_round, seed = KINDS[kind]
    bm, bn = tiles(kind)
    S = world * SL
    q, k, v = structured_shards(S, D, alpha, seed + 100 * world, dtype=dtype)
    case = dict(world=world, kind=kind, dtype=dtype, D=D, S=S, bm=bm, bn=bn, q=q, k=k, v=v, table=HEAD_TABLE if table else None, dense=dense)
    if dense:
        o64, _ = orc.attention_dense_ref(q.double(), k.double(), v.double(), upcast=False)
        case["o_ref"], case["tol"], case["closest"] = [o64] * STEPS, [o_tolerance(kind, o64)] * STEPS, float("inf")
        return case
    chain, case["closest"] = oracle_chain(q, k, v, bm, bn, p_round, head_thr=case["table"])
    case["o_ref"] = [c[0].double() for c in chain]
    case["tol"] = [o_tolerance(kind, o) for o in case["o_ref"]]
    case["read"], case["written"] = [c[2] for c in chain], [c[3] for c in chain]
    if table:                                                  # what a driver that sliced the table one head off would vote with
        case["written_rotated"] = oracle_chain(q, k, v, bm, bn, p_round, head_thr=HEAD_TABLE[1:] + HEAD_TABLE[:1])[0][-1][3]
    return case


def _margin(name, moved, tol):
    print(f"  sensitivity {name}: moves the reference by {moved:.4g}, tolerance {tol:.4g}, margin {moved / tol:.1f}x")
    assert moved > tol, (name, moved, tol)


def check_full_case(case):
    """Input conditions and sensitivity margins of a ``full_case``, against the oracle alone."""
    G, Hl, o, tol = case["world"], H // case["world"], case["o_ref"][-1], case["tol"][-1]
    print(f"full case world={G} {case['kind']} table={case['table'] is not None} dense={case['dense']}: O tolerance {tol:.4g}, "
          f"closest vote to its threshold {case['closest']:.4g}")
    blocks = o.clone()
    blocks[:, :, :Hl], blocks[:, :, Hl:2 * Hl] = o[:, :, Hl:2 * Hl], o[:, :, :Hl]
    _margin("two head blocks exchanged", (blocks - o).abs().max().item(), tol)
    rows = o.clone()
    rows[:, :SL], rows[:, SL:2 * SL] = o[:, SL:2 * SL], o[:, :SL]
    _margin("two row shards exchanged", (rows - o).abs().max().item(), tol)
    if case["dense"]:
        return
    assert case["closest"] >= BORDERLINE, f"a vote lies {case['closest']} from its threshold: take another seed"
    assert case["read"][-1].shape[0] == B
    for r in range(G):
        n, total = listed(case["read"][-1][:, r * Hl:(r + 1) * Hl])
        print(f"  rank {r}: the last step reads {n} of {total} tiles")
        assert 2 <= n < total, (r, n, total)
        if case["table"] is not None:
            assert not torch.equal(case["written"][-1][:, r * Hl:(r + 1) * Hl], case["written_rotated"][:, r * Hl:(r + 1) * Hl]), \
                f"rank {r}: the table rotated by one head writes the same lists"


# ------------------------------------------------------------------------------------------------------------------------- the ring
def ring_order(world, r):
    """The K/V shards in the order rank r meets them: its own, then r - 1, r - 2, ..."""
    return [(r - i) % world for i in range(world)]


@functools.lru_cache(maxsize=None)
def ring_case(world, kind, batch=B, heads=H, sl=SL, table=False, dense=False, reseed=0):
    """Rank r keeps rows [r * sl, (r + 1) * sl) of q; every (r, K/V shard j) pair is one oracle chain; per step the partials are merged
    in fp64. e4m3: every K/V shard has its own k / v descale, every rank its own q descale."""
    orc = _orc()
    dtype, D, alpha, p_round, seed = KINDS[kind]
    bm, bn = tiles(kind)
    fp8 = dtype == F8
    q, k, v = structured_shards(world * sl, D, alpha, seed + 100 * world + 7 * batch + heads + sl + 1000 * reseed, batch, heads,
                                dtype=dtype, sl=sl)
    shard = lambda x, i: x[:, i * sl:(i + 1) * sl].contiguous()                # noqa: E731
    case = dict(world=world, kind=kind, dtype=dtype, D=D, batch=batch, heads=heads, sl=sl, bm=bm, bn=bn, dense=dense,
                table=HEAD_TABLE if table else None, out_dtype=torch.bfloat16 if fp8 else dtype,
                q=[shard(q, i) for i in range(world)], k=[shard(k, i) for i in range(world)], v=[shard(v, i) for i in range(world)],
                descales=shard_descales(world, seed + 1, batch, heads) if fp8 else None)

    def merged(r, pair_descales=None):
        """Per step: (o_ref fp64, out_pt, lse_ref (B,H,sl)); the chains of the pairs; the closest vote."""
        chains, closest = {}, float("inf")
        for j in ring_order(world, r):
            ds = None
            if fp8:
                qd, kd, vd = case["descales"]
                jj = j if pair_descales is None else pair_descales.get(j, j)
                ds = (qd[r], kd[jj], vd[jj])
            if dense and not fp8:
                o64, lse = orc.attention_dense_ref(case["q"][r].double(), case["k"][j].double(), case["v"][j].double(), upcast=False)
                chains[j], c = [(o64, lse, None, None)] * STEPS, float("inf")
            else:
                chains[j], c = oracle_chain(case["q"][r], case["k"][j], case["v"][j], bm, bn, p_round, head_thr=case["table"],
                                            descales=ds, dense=dense)
            closest = min(closest, c)
        steps = []
        for s in range(STEPS):
            outs = torch.stack([chains[j][s][0].double() for j in ring_order(world, r)])
            lses = torch.stack([chains[j][s][1].double().transpose(1, 2) for j in ring_order(world, r)])       # (G, B, sl, H)
            o_ref, lse_ref = orc.attention_combine_ref(outs, lses)
            o_pt = orc.attention_combine_ref(outs.to(case["out_dtype"]).double(), lses)[0].to(case["out_dtype"])
            steps.append((o_ref, o_pt, lse_ref.transpose(1, 2)))
        return steps, chains, closest

    case["merged"] = merged
    case["ranks"] = [merged(r) for r in range(world)]
    case["tol"] = [[o_tolerance(kind, o_ref, o_pt) for o_ref, o_pt, _ in case["ranks"][r][0]] for r in range(world)]
    return case


def check_ring_case(case):
    """Input conditions and sensitivity margins of a ``ring_case``, against the oracle alone."""
    G, sl = case["world"], case["sl"]
    print(f"ring case world={G} {case['kind']} B={case['batch']} H={case['heads']} Sl={sl} table={case['table'] is not None} "
          f"dense={case['dense']}")
    for r in range(G):
        steps, chains, closest = case["ranks"][r]
        o, tol = steps[-1][0], case["tol"][r][-1]
        print(f"  rank {r}: O tolerance {tol:.4g}, closest vote to its threshold {closest:.4g}")
        other = case["ranks"][(r + 1) % G][0][-1][0]
        _margin(f"rank {r}'s rows taken for rank {(r + 1) % G}'s", (other - o).abs().max().item(), tol)
        if case["descales"] is not None:
            j, jj = ring_order(G, r)[:2]
            wrong = case["merged"](r, {j: jj, jj: j})[0][-1][0]
            _margin(f"rank {r}: shards {j} and {jj} paired with each other's descales", (wrong - o).abs().max().item(), tol)
        if case["dense"]:
            continue
        assert closest >= BORDERLINE, f"rank {r}: a vote lies {closest} from its threshold: take another seed"
        for j in range(G):
            rd = chains[j][-1][2]
            assert rd.shape[0] == case["batch"]
            n, total = listed(rd)
            print(f"  rank {r}, state {j}: the last step reads {n} of {total} tiles")
            assert 2 <= n < total, (r, j, n, total)
            for jj in range(j + 1, G):
                assert not torch.equal(chains[j][-1][3], chains[jj][-1][3]), f"rank {r}: states {j} and {jj} hold the same lists"
