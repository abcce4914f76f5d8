"""CPU: ``rows=`` on the V and O passes - the argument checks that need no device, what reaches the C entry point, and the indexing
of the torch references."""
import sys

import pytest
import torch


class _FakeCuda(torch.Tensor):
    """A CPU tensor that says it lives on a GPU: the argument checks run on it, a launch never happens."""
    is_cuda = True


B, S, H, D = 2, 200, 3, 64


@pytest.fixture
def calls(monkeypatch):
    """The (entry, struct, map) of every C call the V and O passes would make, instead of the call."""
    import liteattention_amd  # noqa: F401
    made = []
    monkeypatch.setattr(sys.modules["liteattention_amd.v_prep"], "_call",
                        lambda entry, x, detail, *args: made.append((entry,) + tuple(getattr(a, "_obj", a) for a in args)))
    return made


def test_bad_tables_are_refused_before_any_launch(calls):
    import liteattention_amd as L
    x = torch.randn(B, S, H, D).bfloat16().as_subclass(_FakeCuda)
    lse = torch.zeros(B, H, S)
    ok = torch.arange(137, dtype=torch.int32)
    for rows, exc in ((ok.long(), TypeError), ([0, 1], TypeError), (ok.view(1, 137).expand(3, 137), ValueError),      # [3, S], B = 2
                      (ok.to("meta"), ValueError), (torch.zeros(2 * 137, dtype=torch.int32)[::2], ValueError)):
        for fn in (L.v_colstats, L.attn_unshift, L.attn_out_fp8, L.SmoothedV(tiles=True)):
            with pytest.raises(exc):
                fn(x, rows=rows)
        with pytest.raises(exc):
            L.v_prep_tiles_rows(x, rows)
    with pytest.raises(ValueError):
        L.attn_unshift(x, rows=ok, out=torch.empty(B, S, H, D).bfloat16())                 # out has the table's rows, not o's
    with pytest.raises(ValueError):
        L.attn_unshift(x, lse=lse[..., :137], rows=ok)                                     # lse has o's rows, not the table's
    with pytest.raises(ValueError):
        L.TokenOrder.from_rows(ok, S).restore_output(x)                                     # a pruned order has no inverse
    assert not calls


def test_pruned_table_reaches_the_rows_entry_points(calls):
    import liteattention_amd as L
    x = torch.randn(B, S, H, D).bfloat16().as_subclass(_FakeCuda)
    t = torch.randperm(S)[:137].int().view(1, 137).expand(B, 137).contiguous()
    pv = L.v_prep_tiles_rows(x, t)
    assert pv.shape == (B, 137, H, D) and pv.workspace.numel() == L.v_tiles_bytes(B, H, 137, D)[1]
    out, lse_out = L.attn_unshift(x, lse=torch.zeros(B, H, S), rows=t)
    assert out.shape == (B, 137, H, D) and lse_out.shape == (B, H, 137)
    assert [c[0] for c in calls] == ["la_v_prep_tiles_rows", "la_attn_unshift_rows"]
    for _, a, m in calls:
        assert (a.seqlen, m.src_seqlen, m.batch_stride, m.src_rows, m.positions) == (137, S, 137, t.data_ptr(), None)


def test_references_index_by_rows():
    import liteattention_amd as L
    g = torch.Generator().manual_seed(0)
    x, shift = torch.randn(B, S, H, D, generator=g).bfloat16(), torch.randn(B, H, D, generator=g)
    lse, dot = torch.randn(B, H, S, generator=g), torch.randn(B, H, S, generator=g)
    lse[1, 2, 5] = float("inf")
    for t in (torch.randint(0, S, (260,), generator=g).int(), torch.stack([torch.randperm(S, generator=g)[:137] for _ in range(B)]).int()):
        pick = (lambda v, dim: v.index_select(dim, t.long())) if t.dim() == 1 else \
            (lambda v, dim: torch.stack([v[b].index_select(dim - 1, t[b].long()) for b in range(B)]))
        xg, lg, dg = pick(x, 1), pick(lse, 2), pick(dot, 2)
        assert torch.equal(L.v_prep_tiles_reference(x, shift=shift, rows=t).view(torch.uint8),
                           L.v_prep_tiles_reference(xg, shift=shift).view(torch.uint8))
        assert all(torch.equal(a, b) for a, b in zip(L.v_colstats_reference(x, rows=t), L.v_colstats_reference(xg)))
        (z, ds), lo = L.attn_out_fp8_reference(x, shift, lse=lse, lse_dot=dot, rows=t)
        (z_ref, ds_ref), lo_ref = L.attn_out_fp8_reference(xg, shift, lse=lg, lse_dot=dg)
        assert torch.equal(z, z_ref) and torch.equal(ds, ds_ref) and torch.equal(lo, lo_ref)
