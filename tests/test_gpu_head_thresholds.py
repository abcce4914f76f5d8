"""GPU: per-head vote thresholds (la_fwd_head_thr, la_skip_list_stats_heads, set_head_thresholds, calibrate_head_thresholds).

Workload: ``helpers.fragmented_qkv`` at B = 2, S = 1024, H = 4 over 4 steps (its hot / cold key tiles differ per head), thresholds
-6, -3, -1.5, -0.5 for heads 0 ... 3. The property under test is exact: heads are independent in attention, so head h of a launch with
a table is, bit for bit, head h of the launch whose scalar threshold is the table's value for h - O, LSE and both list buffers, at every
step. So that no comparison passes vacuously the oracle (CPU, once) and every GPU run show first that the heads end on different
listed-tile counts, that tiles are skipped, and that the table's lists are those of no single scalar."""
import ctypes

import pytest
import torch

import error_schedule_common as esc
from helpers import fragmented_qkv

pytestmark = pytest.mark.gpu

B, S, H, STEPS, SEED = 2, 1024, 4, 4, 3
THR = (-6.0, -3.0, -1.5, -0.5)
F8 = torch.float8_e4m3fn

#           id            dtype           D    Hk  list dtype    environment
CONFIGS = {"bf16_d128": (torch.bfloat16, 128, 4, torch.int32, {}),
           "fp16_d64": (torch.float16, 64, 4, torch.int32, {}),
           "bf16_d256": (torch.bfloat16, 256, 4, torch.int32, {}),          # q-tile 128
           "e4m3_d128": (F8, 128, 4, torch.int32, {}),
           "gqa_hk2": (torch.bfloat16, 128, 2, torch.int32, {}),
           "int16_lists": (torch.bfloat16, 128, 4, torch.int16, {}),
           "half_vote": (torch.bfloat16, 128, 4, torch.int32, {"LA_VOTE": "half"}),
           "kernel_v2": (torch.bfloat16, 128, 4, torch.int32, {"LA_FWD_KERNEL": "v2"}),
           "static_sched": (torch.bfloat16, 128, 4, torch.int32, {"LA_SCHED": "static"})}


def _L():
    import liteattention_amd as L
    return L


def _fai():
    from liteattention_amd import flash_attn_interface as fai
    return fai


_INPUTS = {}


def inputs(t, dtype=torch.bfloat16, D=128, Hk=H, batch=None):
    """(q, k, v) of step t on the device (computed once per form and shared: nothing writes to them)."""
    key = (t, dtype, D, Hk)
    if key not in _INPUTS:
        q, k, v = fragmented_qkv(B, S, Hk, D, seed=SEED, step=t, steps=STEPS)
        # GQA: the query heads of a group are the group's own (a query head of another direction sees no hot / cold pattern in these
        # keys and skips nothing at any threshold); what differs between them is their threshold
        q = q.repeat_interleave(H // Hk, dim=2)
        _INPUTS[key] = tuple(x.cuda().to(dtype).contiguous() for x in (q, k, v))
    q, k, v = _INPUTS[key]
    return (q, k, v) if batch is None else tuple(x[batch:batch + 1] for x in (q, k, v))


def drive(thr, dtype=torch.bfloat16, D=128, Hk=H, list_dtype=torch.int32, batch=None):
    """STEPS calls of ``mha_fwd`` on ping-pong lists from "all tiles listed"; ``thr``: a float (the scalar route, ``la_fwd``) or a device
    tensor (``_thr_head``, ``la_fwd_head_thr``). Returns per step (O, LSE, the list read, the list written), all on the device."""
    from liteattention_amd import skip_lists as sl
    fai = _fai()
    bm, bn = fai.get_tile_sizes(D, 1 if dtype == F8 else 2)
    nb = B if batch is None else 1
    lists = sl.new_skip_lists(nb, H, -(-S // bm), -(-S // bn), "cuda", None, list_dtype)
    steps, phase = [], 0
    for t in range(STEPS):
        q, k, v = inputs(t, dtype, D, Hk, batch)
        kw = dict(thr=-1.0, _thr_head=thr) if isinstance(thr, torch.Tensor) else dict(thr=thr)
        rd = lists[phase].clone()
        o, lse, *_ = fai.mha_fwd(q, k, v, attn_read_list=lists[phase], attn_write_list=lists[1 - phase], **kw)
        assert torch.equal(rd, lists[phase])
        steps.append((o, lse, rd, lists[1 - phase].clone()))
        phase = 1 - phase
    return steps


def listed_per_head(lst):
    """torch on the CPU: listed tiles per (batch, head) of a list [B, H, Qt, Kt + 1], by the row rule of the statistics kernels."""
    x = lst.cpu().long()
    kt = x.shape[3] - 1
    n = x[..., 0].clamp(2, kt)
    pairs = x[..., 1:1 + 2 * (kt // 2)].reshape(*x.shape[:3], kt // 2, 2)
    span = (pairs[..., 0] - pairs[..., 1] + 1).clamp(min=0)
    live = 2 * torch.arange(kt // 2) + 2 <= n[..., None]
    return (span * live).sum(dim=(2, 3))


def assert_not_vacuous(table_steps, scalar_steps):
    final = table_steps[-1][3]
    per_head = listed_per_head(final).sum(dim=0)
    total = B * final.shape[2] * (final.shape[3] - 1)
    assert len(set(per_head.tolist())) >= 2, f"every head ends on the same listed-tile count: {per_head.tolist()}"
    assert int(per_head.min()) < total, "no head skips a tile"
    for thr, steps in scalar_steps.items():
        assert not torch.equal(final, steps[-1][3]), f"the table's lists are those of the scalar {thr}"


@pytest.fixture(scope="module")
def oracle_condition():
    """The same three conditions on the CPU oracle, head by head at its own scalar (the oracle keeps a scalar threshold)."""
    from oracle import oracle as orc
    bm, bn = 256, 64
    qt, kt = S // bm, S // bn
    md = orc.expand_must_do_ref([0, 0], bn, kt + 1)
    final = {}
    for thr in THR:
        lists = [orc.init_skip_list_ref(B, qt, kt, H)[0].contiguous() for _ in range(2)]
        phase = 0
        for t in range(STEPS):
            q, k, v = fragmented_qkv(B, S, H, 128, seed=SEED, step=t, steps=STEPS)
            orc.qkskip_fwd(q, k, v, block_m=bm, block_n=bn, read_list=lists[phase], write_list=lists[1 - phase], must_do_list=md, thr=thr)
            phase = 1 - phase
        final[thr] = lists[phase]
    table_final = torch.stack([final[THR[h]][:, h] for h in range(H)], dim=1)
    per_head = listed_per_head(table_final).sum(dim=0)
    assert len(set(per_head.tolist())) >= 2 and int(per_head.min()) < B * qt * kt
    assert all(not torch.equal(table_final, final[thr]) for thr in THR)
    return per_head


@pytest.fixture
def config(request, monkeypatch):
    dtype, D, Hk, list_dtype, env = CONFIGS[request.param]
    for name in ("LA_VOTE", "LA_FWD_KERNEL", "LA_SCHED"):
        monkeypatch.delenv(name, raising=False)
    for name, val in env.items():
        monkeypatch.setenv(name, val)
    return dict(dtype=dtype, D=D, Hk=Hk, list_dtype=list_dtype)


# ---- 1 + 2 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", list(CONFIGS), indirect=True)
def test_head_h_under_a_table_is_head_h_under_its_scalar(config, oracle_condition):
    table = torch.tensor(THR, device="cuda")
    with_table = drive(table, **config)
    scalars = {thr: drive(thr, **config) for thr in THR}
    assert_not_vacuous(with_table, scalars)
    for h, thr in enumerate(THR):
        for t, ((o, lse, rd, wr), (o_s, lse_s, rd_s, wr_s)) in enumerate(zip(with_table, scalars[thr])):
            assert torch.equal(o[:, :, h].view(torch.int16), o_s[:, :, h].view(torch.int16)), (h, t)
            assert torch.equal(lse[:, h].view(torch.int32), lse_s[:, h].view(torch.int32)), (h, t)
            assert torch.equal(rd[:, h], rd_s[:, h]) and torch.equal(wr[:, h], wr_s[:, h]), (h, t)
    # 2: a table of one value is the scalar call, all heads at once
    for thr in (THR[1], THR[3]):
        same = drive(torch.full((H,), thr, device="cuda"), **config)
        for t, (a, b) in enumerate(zip(same, scalars[thr])):
            assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), t
            assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]), t


def test_a_table_with_a_row_per_batch_and_strided_heads():
    """(B, H) with different rows, every second element of a wider buffer: batch b is the B = 1 run of batch b with row b."""
    wide = torch.full((B, 2 * H), 7.0, device="cuda")                # the elements between are never read: positive, they would flag all
    wide[0, ::2] = torch.tensor(THR, device="cuda")
    wide[1, ::2] = torch.tensor(THR[::-1], device="cuda")
    table = wide[:, ::2]
    assert table.stride() == (2 * H, 2)
    both = drive(table)
    assert not torch.equal(both[-1][3][0], both[-1][3][1])
    for b in range(B):
        one = drive(table[b].contiguous(), batch=b)
        for t, (x, y) in enumerate(zip(both, one)):
            assert torch.equal(x[0][b:b + 1].view(torch.int16), y[0].view(torch.int16)), (b, t)
            assert torch.equal(x[1][b:b + 1].view(torch.int32), y[1].view(torch.int32)), (b, t)
            assert torch.equal(x[2][b:b + 1], y[2]) and torch.equal(x[3][b:b + 1], y[3]), (b, t)


def test_minus_infinity_flags_nothing_for_its_head_only():
    table = torch.tensor([float("-inf"), THR[1], float("-inf"), THR[3]], device="cuda")
    steps = drive(table)
    full = steps[0][2]
    for t, (_, _, rd, wr) in enumerate(steps):
        for h in (0, 2):
            assert torch.equal(listed_per_head(wr)[:, h], listed_per_head(full)[:, h]), (t, h)
    assert int(listed_per_head(steps[-1][3])[:, 3].sum()) < int(listed_per_head(full)[:, 3].sum())


# ---- 3: against the oracle ------------------------------------------------------------------------------------------------------------
def test_every_head_matches_the_oracle_at_its_own_scalar():
    from oracle import oracle as orc
    from test_gpu_parity import _compare_lists, _oracle_tol
    bm, bn = _fai().get_tile_sizes(128, 2)
    qt, kt = S // bm, S // bn
    md = orc.expand_must_do_ref([0, 0], bn, kt + 1)
    border = 0
    for t, (o, lse, rd, wr) in enumerate(drive(torch.tensor(THR, device="cuda"))):
        q, k, v = fragmented_qkv(B, S, H, 128, seed=SEED, step=t, steps=STEPS)
        o_all = torch.empty(B, S, H, 128)
        for h, thr in enumerate(THR):
            one = lambda x: x[:, :, h:h + 1].contiguous()      # noqa: E731
            rd_h, wr_h = rd[:, h:h + 1].cpu().contiguous(), wr[:, h:h + 1].cpu().contiguous()
            wr_orc, margins = torch.zeros_like(wr_h), torch.empty(B, 1, qt, kt)
            o_ref, lse_ref, _ = orc.qkskip_fwd(one(q), one(k), one(v), block_m=bm, block_n=bn, read_list=rd_h, write_list=wr_orc,
                                               must_do_list=md, thr=thr, margins=margins)
            o_all[:, :, h:h + 1] = o_ref
            assert (lse[:, h:h + 1].cpu() - lse_ref).abs().max().item() <= 1e-3, (t, h)
            bad, near = _compare_lists(orc, rd_h, wr_h, wr_orc, margins, thr, B)
            assert bad == 0, f"step {t} head {h}: {bad} rows differ from the oracle with no borderline tile"
            border += near
        # O as that file holds it: the call's whole output against the call's whole reference (here put together head by head)
        err, tol = (o.float().cpu() - o_all).abs().max().item(), _oracle_tol(o_all)
        print(f"step {t}: max |O - oracle| = {err:.6f}, tolerance {tol:.6f}")
        assert err <= tol, t
    assert border <= 2


# ---- 4: packed batch ------------------------------------------------------------------------------------------------------------------
def test_packed_batch_with_lists_takes_row_b_for_sequence_b():
    from liteattention_amd import skip_lists as sl
    fai = _fai()
    lens = (512, 768)
    bm, bn = fai.get_tile_sizes(128, 2)
    qt, kt = -(-max(lens) // bm), -(-max(lens) // bn)
    table = torch.tensor([THR, THR[::-1]], device="cuda")
    cu = torch.tensor([0, lens[0], lens[0] + lens[1]], dtype=torch.int32, device="cuda")
    packed = sl.new_skip_lists(2, H, qt, kt, "cuda", None, torch.int32)
    alone = [sl.new_skip_lists(1, H, -(-n // bm), -(-n // bn), "cuda", None, torch.int32) for n in lens]
    phase, skipped = 0, False
    for t in range(STEPS):
        q, k, v = inputs(t)
        seqs = [tuple(x[b:b + 1, :n] for x in (q, k, v)) for b, n in enumerate(lens)]
        qp, kp, vp = (torch.cat([s[i][0] for s in seqs]) for i in range(3))
        o, lse, *_ = fai.mha_fwd(qp, kp, vp, cu_seqlens_q=cu, cu_seqlens_k=cu, max_seqlen_q=max(lens), max_seqlen_k=max(lens),
                                 attn_read_list=packed[phase], attn_write_list=packed[1 - phase], thr=-1.0, _thr_head=table)
        for b, n in enumerate(lens):
            o_b, lse_b, *_ = fai.mha_fwd(*seqs[b], attn_read_list=alone[b][phase], attn_write_list=alone[b][1 - phase], thr=-1.0,
                                         _thr_head=table[b])
            r0 = int(cu[b])
            assert torch.equal(o[r0:r0 + n].view(torch.int16), o_b[0].view(torch.int16)), (t, b)
            assert torch.equal(lse[:, r0:r0 + n].view(torch.int32), lse_b[0].view(torch.int32)), (t, b)
            qb, kb = -(-n // bm), -(-n // bn)
            got, want = packed[1 - phase][b, :, :qb], alone[b][1 - phase][0]
            for h in range(H):
                for m in range(qb):
                    L0 = int(want[h, m, 0])
                    assert torch.equal(got[h, m, :L0 + 1], want[h, m, :L0 + 1]), (t, b, h, m)
            skipped = skipped or int(listed_per_head(want[None]).sum()) < H * qb * kb
        phase = 1 - phase
    assert skipped and not torch.equal(listed_per_head(alone[0][phase]), listed_per_head(alone[0][phase]).flip(1))


# ---- 5: the windowed and the prepared-V routes ----------------------------------------------------------------------------------------
def _class_steps(call, table):
    L = _L()
    att = L.LiteAttention(max_batch_size=B)
    att.set_head_thresholds(table)
    out = []
    for t in range(STEPS):
        o, lse = call(att, t)
        out.append((o, lse, att._skip_list.clone(), att._phase))
    return out


def _same(a, b):
    for t, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x[0].view(torch.int16), y[0].view(torch.int16)) and torch.equal(x[1].view(torch.int32), y[1].view(torch.int32)), t
        assert torch.equal(x[2], y[2]) and x[3] == y[3], t


def test_windowed_call_equals_the_unwindowed_one_and_both_equal_the_functional_route():
    table = torch.tensor(THR, device="cuda")
    plain = _class_steps(lambda att, t: att(*inputs(t), return_softmax_lse=True), table)
    windows = [(0, 1), (1, 2), (3, 1)]                                    # S = 1024: four q-tiles of 256 rows
    windowed = _class_steps(lambda att, t: att.call_windowed(*inputs(t), windows, return_softmax_lse=True), table)
    _same(plain, windowed)
    for (o, lse, lists, phase), (o_f, lse_f, _, wr_f) in zip(plain, drive(table)):      # ... and the class adds nothing to mha_fwd
        assert torch.equal(o.view(torch.int16), o_f.view(torch.int16)) and torch.equal(lse.view(torch.int32), lse_f.view(torch.int32))
        assert torch.equal(lists[phase], wr_f)
    assert int(listed_per_head(plain[-1][2][plain[-1][3]]).sum()) < B * H * 4 * 16


def test_prepared_v_route_equals_the_tensor_route():
    L = _L()
    table = torch.tensor(THR, device="cuda")

    def tensor_route(att, t):
        q, k, v = inputs(t)
        return att(q.to(F8), k.to(F8), L.qk_prep_fp8(v, norm=None), return_softmax_lse=True)

    def tile_route(att, t):
        q, k, v = inputs(t)
        return att(q.to(F8), k.to(F8), L.v_prep_tiles(v), return_softmax_lse=True)

    a, b = _class_steps(tensor_route, table), _class_steps(tile_route, table)
    _same(a, b)
    per_head = listed_per_head(a[-1][2][a[-1][3]]).sum(dim=0)
    assert len(set(per_head.tolist())) >= 2 and int(per_head.min()) < B * 4 * 16


# ---- 6: graph -------------------------------------------------------------------------------------------------------------------------
def test_a_captured_call_follows_the_table_in_place():
    from liteattention_amd import skip_lists as sl
    fai = _fai()
    q, k, v = inputs(1)
    bm, bn = fai.get_tile_sizes(128, 2)
    read = drive(-2.0)[0][3]                                              # a list with holes: what step 0 wrote at -2
    tables = [torch.tensor(THR, device="cuda"), torch.tensor(THR[::-1], device="cuda"), torch.full((H,), -1.0, device="cuda")]

    def eager(table):
        wr = sl.new_skip_lists(B, H, S // bm, S // bn, "cuda", None, torch.int32)[1]
        o, lse, *_ = fai.mha_fwd(q, k, v, attn_read_list=read, attn_write_list=wr, thr=-1.0, _thr_head=table)
        return o.clone(), lse.clone(), wr

    want = [eager(t) for t in tables]
    assert not torch.equal(want[0][2], want[1][2])
    live = tables[2].clone()
    wr_g = sl.new_skip_lists(B, H, S // bm, S // bn, "cuda", None, torch.int32)[1]
    fai.mha_fwd(q, k, v, attn_read_list=read, attn_write_list=wr_g, thr=-1.0, _thr_head=live)      # warm-up before the capture
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o_g, lse_g, *_ = fai.mha_fwd(q, k, v, attn_read_list=read, attn_write_list=wr_g, thr=-1.0, _thr_head=live)
    for other, (o, lse, wr) in zip(tables, want):
        live.copy_(other)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(o_g.view(torch.int16), o.view(torch.int16)) and torch.equal(lse_g.view(torch.int32), lse.view(torch.int32))
        n = wr[..., :1].long()                                             # a row is [L, L entries]: what lies behind is not written
        live_part = torch.arange(wr.shape[-1], device="cuda") <= n
        assert torch.equal(wr_g[..., 0], wr[..., 0]) and torch.equal(wr_g * live_part, wr * live_part)


# ---- 7: listed tiles per head ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("list_dtype", [torch.int32, torch.int16])
def test_skip_list_stats_heads(list_dtype):
    L = _L()
    steps = drive(torch.tensor(THR, device="cuda"), list_dtype=list_dtype)
    for t, (_, _, rd, wr) in enumerate(steps):
        for lst in (rd, wr):
            got = L.skip_list_stats_heads(lst)
            assert got.dtype == torch.int64 and tuple(got.shape) == (B, H)
            assert torch.equal(got.cpu(), listed_per_head(lst)), t
            assert int(got.sum()) == int(L.skip_list_stats(lst)[0])
            again = torch.full_like(got, -1)
            rc = L._cabi.load().la_skip_list_stats_heads(lst.data_ptr(), lst.element_size(), B, H, lst.shape[2], lst.shape[3] - 1,
                                                         again.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0 and torch.equal(again, got)                     # every element written; bit-equal across launches
    one = L.skip_list_stats_heads(steps[-1][3], batch=1)
    assert tuple(one.shape) == (1, H) and torch.equal(one.cpu(), listed_per_head(steps[-1][3])[:1])
    # rows the rule bends: a length below 2 counts as 2, one above Kt is clamped, a negative span counts 0
    kt = 16
    odd = torch.zeros(1, 2, 3, kt + 1, dtype=list_dtype, device="cuda")
    odd[0, 0, 0, :3] = torch.tensor([0, 9, 4])                             # length 0 -> the first range is walked: 6
    odd[0, 0, 1, :5] = torch.tensor([4, 3, 5, 2, 1])                       # 3 - 5 + 1 < 0 -> 0, then 2
    odd[0, 0, 2, 0] = 100                                                  # clamped to Kt = 16: eight pairs of (0, 0) -> 8
    odd[0, 1, 0, :3] = torch.tensor([2, 15, 0])                            # 16
    assert L.skip_list_stats_heads(odd).tolist() == [[6 + 2 + 8, 16 + 1 + 1]]
    assert int(L.skip_list_stats(odd)[0]) == 34
    att = L.LiteAttention(max_batch_size=B, list_dtype=list_dtype)
    assert att.get_skip_fraction_heads() is None
    att.set_head_thresholds(torch.tensor(THR, device="cuda"))
    for t in range(2):
        att(*inputs(t))
    frac = att.get_skip_fraction_heads()
    assert frac.is_cuda and tuple(frac.shape) == (B, H)
    want = 1.0 - listed_per_head(att.current_read_list()).double() / (4 * 16)
    assert torch.allclose(frac.cpu().double(), want, atol=1e-6)
    assert abs(float(frac.mean()) - att.get_skip_fraction()) < 1e-6


# ---- 8: the calibrator on the kernels --------------------------------------------------------------------------------------------------
def test_calibrated_table_replays_bit_for_bit_and_never_skips_less_than_the_scalar_schedule():
    L = _L()
    from liteattention_amd import calibration as cal
    qkv_at = lambda t: inputs(t)      # noqa: E731
    dense = [L.flash_attn_func(*qkv_at(t)) for t in range(STEPS)]
    # bounds by error_schedule_common's rule: a fraction of the error of the constant threshold -0.001 at every step
    att = L.LiteAttention(threshold=esc.HI_THR, max_batch_size=B)
    e_hi = [float(cal.output_error(att(*qkv_at(t)), dense[t]).rel_l1.max()) for t in range(STEPS)]
    bounds = esc.bounds_from(e_hi)
    assert all(b > 0 for b in bounds)

    class Recording(cal.LiteAttentionBackend):
        """The default backend; keeps what every call of a committed run returned (probes are overwritten by the commit that follows)."""
        def __init__(self):
            super().__init__(qkv_at, max_batch_size=B)
            self.last = {}

        def step(self, t, thr):
            rd = self.att._phase if self.att._skip_list is not None else 0
            o, lse = (self.att.set_head_thresholds(thr), self.att(*self.qkv_at(t), return_softmax_lse=True))[1]
            self.last[t] = (o, lse, self.att._skip_list.clone(), self.att._phase, rd)
            return o

    be = Recording()
    table, trace = cal.calibrate_head_thresholds(qkv_at, STEPS, bounds, iters=6, max_batch_size=B, backend=be)
    assert table.is_cuda and table.dtype == torch.float32 and tuple(table.shape) == (STEPS, H)
    committed = dict(be.last)
    # replay through set_head_thresholds: O, LSE and lists of the committed run, bit for bit
    att = L.LiteAttention(max_batch_size=B)
    att.set_head_thresholds(table)
    for t in range(STEPS):
        assert torch.equal(att.current_head_thresholds(), table[t])
        o, lse = att(*qkv_at(t), return_softmax_lse=True)
        o_c, lse_c, lists_c, phase_c, _ = committed[t]
        assert torch.equal(o.view(torch.int16), o_c.view(torch.int16)) and torch.equal(lse.view(torch.int32), lse_c.view(torch.int32)), t
        assert torch.equal(att._skip_list, lists_c) and att._phase == phase_c, t
        err = cal.output_error(o, dense[t]).rel_l1.amax(dim=0)
        assert torch.equal(err, trace[t]["error"]) and torch.equal(trace[t]["threshold"], table[t]), t
        met = trace[t]["bound_met"]
        assert bool((err[met] <= bounds[t]).all()), t
        assert tuple(trace[t]["skip_fraction"].shape) == (H,)
    # the scalar schedule under the same bounds, lo, hi and iters: at step 0 every tile is read, so the vote is an exact comparison
    # and the highest passing grid point of a head is at least that of all heads together
    sched, _ = cal.calibrate_error_schedule(qkv_at, STEPS, bounds, reduce="max", iters=6, max_batch_size=B)
    assert bool((table[0] >= sched[0] - 1e-6).all()), (table[0].tolist(), sched[0])
    scalar_att = L.LiteAttention(max_batch_size=B)
    scalar_att.set_threshold_schedule(sched)
    scalar_att(*qkv_at(0))
    mine = listed_per_head(committed[0][2][committed[0][3]]).sum(dim=0)
    theirs = listed_per_head(scalar_att.current_read_list()).sum(dim=0)
    assert bool((mine <= theirs).all()), (mine.tolist(), theirs.tolist())
