"""GPU: the V and O passes with a row map (la_v_prep_tiles_rows, la_v_colstats_rows, la_attn_unshift_rows, la_attn_unshift_fp8_rows).

Every comparison is bit equality, no tolerance: a fused pass does per element what the torch gather and the unmapped pass do one after
the other - an index_select is an exact copy, amax an order-free maximum of bit patterns, and the column partials are cut from the
table's length and summed in table order. Shapes: 200 source rows; tables of 200 (a permutation), 137 (pruned: a ragged last tile of
64 and of 32) and 260 entries (repeats, more rows than the source, several workgroups); one [S] table for B = 1, two different ones
[B, S] for B = 2; every head dim of the tile writer; one case whose heads are not contiguous. The O passes run 3 and 6 query heads
over 3 shift vectors (6: two heads share one), with an empty row of either sign at rows the tables move."""
import pytest
import torch

pytestmark = pytest.mark.gpu
S_SRC = 200
TABLES = ["perm", "pruned", "repeats"]
#         D    dtype          B  strided heads
CASES = [(D, dt, B, False) for D in (64, 96, 128, 256) for dt, B in ((torch.bfloat16, 1), (torch.float32, 2))] + \
        [(128, torch.bfloat16, 2, True)]
IDS = [f"d{D}-{str(dt)[6:]}-b{B}{'-strided' if st else ''}" for D, dt, B, st in CASES]
cases = pytest.mark.parametrize("D,dtype,B,strided", CASES, ids=IDS)
tables = pytest.mark.parametrize("table", TABLES)


def make_table(kind, B):
    """int32 [S] for B = 1, [B, S] with different rows for B = 2; seeded."""
    g = torch.Generator().manual_seed(7)
    one = {"perm": lambda: torch.randperm(S_SRC, generator=g), "pruned": lambda: torch.randperm(S_SRC, generator=g)[:137],
           "repeats": lambda: torch.randint(0, S_SRC, (260,), generator=g)}[kind]
    t = one() if B == 1 else torch.stack([one() for _ in range(B)])
    return t.int().cuda()


def take(t, rows, dim):
    if rows.dim() == 1:
        return t.index_select(dim, rows.long())
    return torch.stack([t[b].index_select(dim - 1, rows[b].long()) for b in range(t.shape[0])])


def make_x(B, H, D, dtype, strided, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, S_SRC, H, (2 if strided else 1) * D, generator=g) * 3 + 0.5).to(dtype).cuda()
    return x[..., :D]


@tables
@cases
def test_v_passes(D, dtype, B, strided, table):
    import liteattention_amd as L
    H, t = 3, make_table(table, B)
    v = make_x(B, H, D, dtype, strided)
    g = torch.Generator().manual_seed(1)
    shift, descale = torch.randn(B, H, D, generator=g).cuda(), (0.01 + torch.rand(B, H, generator=g)).cuda()
    vg = take(v, t, 1)
    mean, amax = L.v_colstats(v, rows=t)
    mean_ref, amax_ref = L.v_colstats(vg)
    assert torch.equal(mean, mean_ref) and torch.equal(amax, amax_ref)
    am, am_ref = torch.zeros(B, H).cuda(), torch.zeros(B, H).cuda()
    pv = L.v_prep_tiles_rows(v, t, shift=shift, descale=descale, amax_out=am)
    pv_ref = L.v_prep_tiles(vg, shift=shift, descale=descale, amax_out=am_ref)
    n = L.v_tiles_bytes(B, H, t.shape[-1], D)[0]
    assert pv.shape == pv_ref.shape == (B, t.shape[-1], H, D)
    assert torch.equal(pv.workspace[:n], pv_ref.workspace[:n]) and torch.equal(am, am_ref)


def make_o(B, H, D, dtype, strided):
    """o, shift over 3 kv heads, lse with an empty row of each sign, lse_dot."""
    o = make_x(B, H, D, torch.bfloat16 if dtype == torch.bfloat16 else torch.float16, strided, seed=2)
    g = torch.Generator().manual_seed(3)
    shift = torch.randn(B, 3, D, generator=g).cuda()
    lse, dot = torch.randn(B, H, S_SRC, generator=g).cuda(), torch.randn(B, H, S_SRC, generator=g).cuda()
    lse[0, 1, 7], lse[-1, 0, 150] = float("-inf"), float("inf")
    return o, shift, lse, dot


@pytest.mark.parametrize("H", [3, 6])
@tables
@cases
def test_attn_unshift(D, dtype, B, strided, table, H):
    import liteattention_amd as L
    d = make_table(table, B)
    o, shift, lse, dot = make_o(B, H, D, dtype, strided)
    out, lse_out = L.attn_unshift(o, shift, lse=lse, lse_dot=dot, out_dtype=dtype, rows=d)
    ref, lse_ref = L.attn_unshift(o, shift, lse=lse, lse_dot=dot, out_dtype=dtype)
    assert torch.equal(out, take(ref, d, 1)) and torch.equal(lse_out, take(lse_ref, d, 2))
    assert torch.equal(L.attn_unshift(o, shift, out_dtype=dtype, rows=d), take(L.attn_unshift(o, shift, out_dtype=dtype), d, 1))  # no lse
    plain, lse_plain = L.attn_unshift(o, lse=lse, rows=d)                                              # restore + restore_lse
    assert torch.equal(plain, take(L.attn_unshift(o, lse=lse), d, 1)) and torch.equal(lse_plain, take(lse, d, 2))


@pytest.mark.parametrize("static", [False, True], ids=["dynamic", "static"])
@pytest.mark.parametrize("H", [3, 6])
@tables
@cases
def test_attn_out_fp8(D, dtype, B, strided, table, H, static):
    import liteattention_amd as L
    d = make_table(table, B)
    o, shift, lse, dot = make_o(B, H, D, dtype, strided)
    kw = dict(lse=lse, lse_dot=dot, heads_per_scale=H if D < 256 else 1)
    am, am_ref = torch.zeros(B).cuda(), torch.zeros(B).cuda()
    ds = torch.full((B,), 0.03).cuda() if static else None
    r, lse_out = L.attn_out_fp8(o, shift, rows=d, descale=ds, amax_out=am if static else None, **kw)
    ref, lse_ref = L.attn_out_fp8(o, shift, descale=ds, **kw)
    assert torch.equal(r.data.view(torch.uint8), take(ref.data.view(torch.uint8), d, 1)) and torch.equal(lse_out, take(lse_ref, d, 2))
    if static:                                             # the running maximum is one of the rows the table names: the gathered input's
        L.attn_out_fp8(take(o, d, 1), shift, lse=take(lse, d, 2), lse_dot=take(dot, d, 2), heads_per_scale=kw["heads_per_scale"],
                       descale=ds, amax_out=am_ref)
        assert torch.equal(am, am_ref)
    else:
        assert torch.equal(r.descale, take(ref.descale, d, 1))


def test_restore_output_is_restore_and_restore_lse():
    import liteattention_amd as L
    order = L.brick_order((2, 10, 10), ((1, 4, 4),), device="cuda")
    o, _, lse, _ = make_o(2, 3, 128, torch.bfloat16, False)
    out, lse_out = order.restore_output(o, lse)
    want = order.restore(o)
    want[0, order.src_rows[7].item(), 1] = 0               # the empty rows of make_o: zeros, where restore() copies
    want[1, order.src_rows[150].item(), 0] = 0
    assert torch.equal(out, want) and torch.equal(lse_out, order.restore_lse(lse))
