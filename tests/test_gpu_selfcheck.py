"""GPU: one launch, two judges — the full-size checker (tools/selfcheck.py) and the CPU oracle on the SAME kernel results.

The checker alone judges the launches the oracle cannot finish (S = 75 600). tests/test_selfcheck_cpu.py pins it to the oracle on
the host; here both look at what the kernels really return, at a size the oracle still finishes (S ~ 6 100, the fragmenting
generator, thr = -3, 4 ping-pong steps):

  * the oracle, walking the same read list, under the tolerances of tests/test_gpu_fragmented.py (``_setup`` / ``_compare_lists``);
  * sampled_row_check (all heads, 1 024 rows, on the device) and vote_writer_check (every item);
  * per item the checker's expected row is the oracle's written row unless the ORACLE's margins hold a tile within 1e-3 of thr;
  * both judges flag the same rows;
  * the checker's decision margins (fp32 torch on the device) stay within margin_tol = 1e-3 of the oracle's on every computed tile:
    the borderline window must be wider than the checker's own summation noise.

Checker bounds on these PEAKED rows: bf16 |O - ref| <= 2^-7 max|ref| + 1e-4 (one bf16 ulp at the maximum under the lazy rescale:
tests/test_gpu_fragmented.py docstring, and what tests/test_gpu_denoise_lists.py uses), fp16 the default 2^-8 max|ref| + 1e-4, e4m3
0.05 max|ref| + 1e-3; |LSE - ref| <= 2e-4 throughout (fp8 runs in its default form, fp32 row sums).

And one faulted copy at the headline shape (B=1, S=75 600, H=40, bf16, imposed 42 % band): a copy of the kernel's result in which one
q-tile was recomputed in fp32 torch WITHOUT one listed tile must fail sampled_row_check at the headline test's bounds, where the true
result passes. The tile is chosen from the fp32 reference alone so that it moves a sampled row's LSE by >= 10x the bound.
"""
import math

import pytest
import torch

from helpers import fragmented_qkv
from test_gpu_parity import _compare_lists
from test_selfcheck_cpu import gqa_heads

pytestmark = pytest.mark.gpu
F8 = torch.float8_e4m3fn
STEPS, THR, MARGIN_TOL = 4, -3.0, 1e-3

CASES = {
    # name: env, dtype, D, Sq, Sk, H, Hk, must-do tokens
    "bf16-d128": ({}, "bf16", 128, 6100, 6100, 4, 4, None),
    "bf16-d128-half-vote": ({"LA_VOTE": "half"}, "bf16", 128, 6100, 6100, 4, 4, None),
    "fp16-d64": ({}, "fp16", 64, 6100, 6100, 4, 4, None),
    "e4m3-d128": ({}, "fp8", 128, 6100, 6100, 4, 4, None),
    "gqa-4-2-ragged": ({}, "bf16", 128, 4900, 6087, 4, 2, None),
    "must-do-3-ranges": ({}, "bf16", 128, 6100, 6100, 4, 4, (5900, 5200, 3050, 2650, 300, 0)),
}


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for name in ("LA_VOTE", "LA_FWD_KERNEL", "LA_SCHED", "LA_LIST_DTYPE", "LA_FP8_P"):
        monkeypatch.delenv(name, raising=False)


def _checker_bounds(dtype):
    if dtype == "fp8":
        return dict(o_rtol=0.05, o_atol=1e-3, lse_atol=2e-4)
    return dict(o_rtol=2.0 ** -7 if dtype == "bf16" else 2.0 ** -8, o_atol=1e-4, lse_atol=2e-4)


@pytest.mark.parametrize("name", list(CASES))
def test_one_launch_two_judges(name, monkeypatch):
    env, dtype, D, Sq, Sk, H, Hk, md_tokens = CASES[name]
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    from test_gpu_fragmented import _setup
    from tools import selfcheck as sc
    from liteattention_amd import skip_lists as sl
    from liteattention_amd.flash_attn_interface import mha_fwd
    L, orc, bm, bn, cast, p_round, tol, lse_tol = _setup(dtype, D)
    B = 1
    Qt, Kt = math.ceil(Sq / bm), math.ceil(Sk / bn)
    torch_dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp8": F8}[dtype]
    lists = L.LiteAttention.init_skip_list(B, Sq, H, D, False, torch_dtype, "cuda", seq_len_k=Sk)
    assert tuple(lists.shape) == (2, B, H, Qt, Kt + 1)
    md_dev = sl.must_do_row(list(md_tokens) if md_tokens else [0, 0], bn, Kt + 1, "cuda")
    md_cpu = md_dev.cpu()
    assert torch.equal(md_cpu, orc.expand_must_do_ref(list(md_tokens) if md_tokens else [0, 0], bn, Kt + 1))
    items = [(h, m) for h in range(H) for m in range(Qt)]
    margins = torch.empty(B, H, Qt, Kt)
    worst_margin, max_len = 0.0, 0
    counts = dict(borderline_oracle=0, borderline=0, explained=0, unexplained=0, unenumerated=0)
    for step in range(STEPS):
        q, k, v = fragmented_qkv(B, Sq, Hk, D, seed=5, step=step, steps=STEPS, dtype=torch.float32, Sk=Sk)
        if H != Hk:
            q = gqa_heads(q, H // Hk)
        q, k, v = [cast(x) for x in (q, k, v)]
        qd, kd, vd = q.cuda(), k.cuda(), v.cuda()
        rd_dev, wr_dev = lists[step % 2], lists[1 - step % 2]
        wr_dev.fill_(-7)                                                   # the kernel must write every live entry
        out, lse, *_ = mha_fwd(qd, kd, vd, attn_read_list=rd_dev, attn_must_do_list=md_dev, attn_write_list=wr_dev, thr=THR,
                               _must_do_is_1d=True)
        rd, wr = rd_dev.cpu(), wr_dev.cpu()
        max_len = max(max_len, int(rd[..., 0].max()))

        # judge 1: the oracle on the same read list
        wr_orc = torch.zeros_like(wr)
        o_ref, lse_ref, n_tiles = orc.qkskip_fwd(q, k, v, block_m=bm, block_n=bn, read_list=rd, write_list=wr_orc,
                                                 must_do_list=md_cpu, thr=THR, margins=margins, p_round=p_round)
        assert n_tiles == orc.listed_tiles(rd)
        err_o, err_l = (out.float().cpu() - o_ref).abs().max().item(), (lse.cpu() - lse_ref).abs().max().item()
        print(f"{name} step {step}: vs oracle |dO| {err_o:.3e} (<= {tol(o_ref):.3e}) |dLSE| {err_l:.3e} (<= {lse_tol:.3e})")
        assert err_o <= tol(o_ref), f"step {step}"
        assert err_l <= lse_tol, f"step {step}"
        bad, border = _compare_lists(orc, rd, wr, wr_orc, margins, THR, B)
        assert bad == 0, f"step {step}: {bad} rows differ from the oracle with no borderline tile"
        counts["borderline_oracle"] += border

        # judge 2: the checker, on the device
        res = sc.sampled_row_check(qd, kd, vd, out, lse, rd_dev, bm, bn, heads=range(H), n_rows=1032, **_checker_bounds(dtype))
        print(f"{name} step {step}: sampled_row_check {res}")
        assert res["ok"] and res["rows"] >= H * 1024, (step, res)
        vw = sc.vote_writer_check(qd, kd, rd_dev, wr_dev, THR, bm, bn, items, must_do_row=md_cpu if md_tokens else None,
                                  details=True)
        print(f"{name} step {step}: vote_writer_check", {k_: v_ for k_, v_ in vw.items() if k_ != "details"})
        assert vw["ok"] and vw["items"] == len(items) and vw["unexplained"] == 0, (step, vw)
        counts["borderline"] += vw["borderline"]
        counts["unexplained"] += vw["unexplained"]
        counts["unenumerated"] += vw["unenumerated"]

        # the two judges against each other, item by item
        flagged_oracle, flagged_checker = set(), set()
        for (h, m), d in vw["details"].items():
            mine, theirs = d["margin"], margins[0, h, m]
            assert torch.equal(torch.isnan(mine), torch.isnan(theirs)), (step, h, m)          # the same tiles were voted on
            live = ~torch.isnan(mine)
            if bool(live.any()):
                worst_margin = max(worst_margin, (mine - theirs)[live].abs().max().item())
            e = wr_orc[0, h, m]
            oracle_row = e[: int(e[0]) + 1].tolist()
            close = bool(live.any()) and bool(((theirs[live] - THR).abs() < MARGIN_TOL).any())
            if d["want"] != oracle_row:
                assert close, (step, h, m, d["want"], oracle_row)
            if wr[0, h, m, : len(oracle_row)].tolist() != oracle_row:
                flagged_oracle.add((h, m))
            if d["status"] != "equal":
                flagged_checker.add((h, m))
                counts["explained"] += d["status"] == "explained"
        # a row the judges disagree on: each saw a close vote fall on another side, which only a close vote of the oracle allows
        for h, m in flagged_oracle ^ flagged_checker:
            theirs = margins[0, h, m]
            theirs = theirs[~torch.isnan(theirs)]
            assert bool(((theirs - THR).abs() < MARGIN_TOL).any()), (step, h, m)
            assert vw["details"][(h, m)]["want"] != wr_orc[0, h, m, : int(wr_orc[0, h, m, 0]) + 1].tolist(), (step, h, m)
    print(f"{name}: max |checker margin - oracle margin| = {worst_margin:.3e}; rows {counts}; longest read row {max_len // 2} ranges")
    assert worst_margin < MARGIN_TOL, f"the checker's margins differ from the oracle's by {worst_margin:.3e}: the borderline window " \
                                      f"of {MARGIN_TOL} is narrower than the checker's own summation noise"
    assert max_len >= 20, f"longest read row holds {max_len // 2} ranges: the lists did not fragment"
    assert counts["borderline_oracle"] <= 4 and counts["borderline"] <= 4, counts


def test_a_faulted_copy_of_the_headline_result_is_rejected():
    import liteattention_amd as L
    from tools import selfcheck as sc
    S, H, D, sparsity, heads, n_rows = 75600, 40, 128, 0.42, (0, 17, 39), 256
    bounds = dict(o_rtol=2.0 ** -8, o_atol=1e-4, lse_atol=2e-4)            # tests/test_gpu_headline.py, bf16
    g = torch.Generator(device="cuda").manual_seed(1234)
    q, k, v = [torch.randn(1, S, H, D, device="cuda", generator=g, dtype=torch.float32).to(torch.bfloat16) for _ in range(3)]
    bm, bn = L.get_tile_sizes(D, 2)
    qt, kt = -(-S // bm), -(-S // bn)
    att = L.LiteAttention(max_batch_size=1)
    att.threshold = float("-inf")
    att._get_read_write_lists(q, k)
    att._phase = 0
    sc.impose_lists(att, sc.banded_rows(qt, kt, bm, bn, sparsity))
    read = att._skip_list[0].clone()
    out, lse = att(q, k, v, return_softmax_lse=True)

    # from the fp32 reference alone: the sampled row and listed non-first tile whose omission moves that row's LSE furthest
    rows = sc.sample_rows(S, n_rows, bm, seed=1).cuda()
    scale = D ** -0.5
    best = (0.0, None)
    for h in heads:
        s = (q[0, rows, h].float() @ k[0, :, h].float().T) * scale                              # [n, S]
        s = torch.nn.functional.pad(s, (0, kt * bn - S), value=float("-inf"))
        listed = sc.lists_to_bitmap(read[0, h])[rows // bm]                                     # [n, kt]
        tile_lse = torch.logsumexp(s.view(-1, kt, bn), dim=-1).masked_fill(~listed, float("-inf"))
        row_lse = torch.logsumexp(tile_lse, dim=-1, keepdim=True)
        share = torch.exp(tile_lse - row_lse)
        share[:, kt - 1] = 0.0                                                                  # not the first walked tile
        moved = -torch.log1p(-share)                                                            # |LSE without the tile - LSE|
        top, idx = moved.flatten().max(0)
        if top.item() > best[0]:
            best = (top.item(), (h, int(rows[idx // kt]), int(idx % kt)))
    moved, (h, row, tile) = best
    print(f"faulted copy: head {h}, row {row} (q-tile {row // bm}), tile {tile} left out moves the LSE by {moved:.3e} = "
          f"{moved / bounds['lse_atol']:.1f} x the bound")
    assert moved >= 10 * bounds["lse_atol"], moved

    m = row // bm
    r0, r1 = m * bm, min((m + 1) * bm, S)
    mask = sc.listed_key_mask(read[0, h, m].tolist(), bn, S, "cuda")
    assert bool(mask[tile * bn: (tile + 1) * bn].all())
    mask[tile * bn: (tile + 1) * bn] = False
    s = ((q[0, r0:r1, h].float() @ k[0, :, h].float().T) * scale).masked_fill(~mask, float("-inf"))
    out_f, lse_f = out.clone(), lse.clone()
    out_f[0, r0:r1, h] = (torch.softmax(s, dim=-1) @ v[0, :, h].float()).to(out.dtype)
    lse_f[0, h, r0:r1] = torch.logsumexp(s, dim=-1)

    true = sc.sampled_row_check(q, k, v, out, lse, read, bm, bn, heads=heads, n_rows=n_rows, **bounds)
    copy = sc.sampled_row_check(q, k, v, out_f, lse_f, read, bm, bn, heads=heads, n_rows=n_rows, **bounds)
    print(f"faulted copy: true {true}\nfaulted copy: copy {copy}")
    assert true["ok"], true
    assert not copy["ok"], copy
