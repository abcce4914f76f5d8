"""CPU: tests/lockstep_ranks.py - G ranks as threads of one process, collectives as plain copies - against REAL gloo worlds of 2 and 3.
The harness restates collectives, so before tests/test_gpu_parallel_ranks.py relies on it the three drivers of
liteattention_amd.parallel must give under it, bit for bit, what they give over gloo (spawned as tests/test_distributed_cpu.py does,
with that file's stand-in attention functions: the eager oracle through the ``attention_fn`` seams). Broken callers must end in an
exception inside the timeout, never in a hang."""
import os
import socket
import sys
import threading
import time

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import lockstep_ranks as ls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S, H, D = 2, 96, 6, 32                 # as tests/test_distributed_cpu.py; 96 rows divide by 2 and 3
WINDOWS = [(0, 2), (2, 3), (5, 1)]        # 6 q-tiles of 16 rows, uneven windows: B > 1 makes every window's rows non-contiguous


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def driver_cases(rank, world, group):
    """Every exchange of the three drivers on one rank of ``group``; returns {name: tensor}. Runs unchanged in a gloo process and in a
    lockstep thread."""
    from liteattention_amd.parallel import HeadShardedLiteAttention, RingSeqParallelLiteAttention, UlyssesLiteAttention
    from oracle import oracle as orc

    def stand_in(q, k, v, scale=None, **kw):
        return orc.attention_dense_ref(q, k, v, softmax_scale=scale)[0]

    def windowed_stand_in(q, k, v, windows, hook, scale=None, **kw):
        out = orc.attention_dense_ref(q, k, v, softmax_scale=scale)[0]
        for i, (t0, n) in enumerate(windows):
            hook(i, out, t0 * 16, min(q.shape[1], (t0 + n) * 16))
        return out

    used = []

    def partial_attention(qq, kk, vv, split_idx, scale=None):
        used.append(split_idx)
        return orc.attention_dense_ref(qq, kk, vv, softmax_scale=scale)

    def combine(outs, lses):
        return orc.attention_combine_ref(outs, lses.transpose(2, 3))[0]

    g = torch.Generator().manual_seed(0)                       # the same full tensors on every rank
    q, k, v = [torch.randn(B, S, H, D, generator=g) for _ in range(3)]
    res = {}
    att = HeadShardedLiteAttention(num_heads=H, max_batch_size=B, process_group=group, attention_fn=stand_in)
    assert (att.world, att.rank) == (world, rank)
    res["hs_plain"] = att(att.shard(q), att.shard(k), att.shard(v))
    over = HeadShardedLiteAttention(num_heads=H, max_batch_size=B, process_group=group, overlap_windows=3,
                                    windowed_attention_fn=windowed_stand_in, q_tile_rows=16)
    over.q_windows = lambda q_: WINDOWS
    blocks = over(over.shard(q), over.shard(k), over.shard(v))
    for i, blk in enumerate(blocks):
        res[f"hs_over_block{i}"] = blk
    res["hs_over"] = HeadShardedLiteAttention.to_bshd(blocks)
    Sl = S // world
    rows = slice(rank * Sl, (rank + 1) * Sl)
    ql, kl, vl = [x[:, rows].contiguous() for x in (q, k, v)]
    uly = UlyssesLiteAttention(num_heads=H, max_batch_size=B, process_group=group, attention_fn=stand_in)
    res["seq_to_head"] = uly.seq_to_head(ql)
    res["head_to_seq"] = uly.head_to_seq(att.shard(k).contiguous())
    res["ulysses"] = uly(ql, kl, vl)
    ring = RingSeqParallelLiteAttention(max_batch_size=B, process_group=group, attention_fn=partial_attention, combine_fn=combine)
    res["ring"] = ring(ql, kl, vl)
    res["ring_used"] = torch.tensor(used)
    return {name: t.clone() for name, t in res.items()}


def _gloo_worker(rank, world, port, tmpdir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.save(driver_cases(rank, world, dist.group.WORLD), os.path.join(tmpdir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_drivers_under_the_harness_are_bit_equal_to_a_gloo_world(world, tmp_path):
    mp.spawn(_gloo_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    gloo = [torch.load(os.path.join(tmp_path, f"rank{r}.pt")) for r in range(world)]
    with ls.distributed() as group:
        mine = ls.run_ranks(world, lambda rank: driver_cases(rank, world, group), timeout_s=30.0)
    from oracle import oracle as orc
    g = torch.Generator().manual_seed(0)
    q, k, v = [torch.randn(B, S, H, D, generator=g) for _ in range(3)]
    ref = orc.attention_dense_ref(q, k, v)[0]
    Sl, Hl = S // world, H // world
    for r in range(world):
        assert sorted(mine[r]) == sorted(gloo[r]) and len(mine[r]) == 10
        for name in gloo[r]:
            assert mine[r][name].dtype == gloo[r][name].dtype and torch.equal(mine[r][name], gloo[r][name]), (r, name)
        assert mine[r]["ring_used"].tolist() == [(r - i) % world for i in range(world)]       # own shard first, then r-1, r-2, ...
        # and both are the right answer, not merely the same one
        assert torch.equal(mine[r]["seq_to_head"], q[:, :, r * Hl:(r + 1) * Hl])
        assert torch.equal(mine[r]["head_to_seq"], k[:, r * Sl:(r + 1) * Sl])
        assert mine[r]["hs_plain"].shape == (world, B, S, Hl, D) and mine[r]["hs_over_block1"].shape == (world, B, 48, Hl, D)
        for name in ("hs_over", "ulysses", "ring"):
            want = ref if name == "hs_over" else ref[:, r * Sl:(r + 1) * Sl]
            assert torch.allclose(mine[r][name], want, atol=1e-5), (r, name)


# ------------------------------------------------------------------------------------------------------------ the harness itself
def test_torch_distributed_is_untouched_outside_the_context():
    before = {name: getattr(dist, name) for name in ls.PATCHED}
    with ls.distributed() as group:
        assert group is ls.GROUP and all(getattr(dist, name) is getattr(ls, name) for name in ls.PATCHED)
    assert all(getattr(dist, name) is obj for name, obj in before.items())
    with pytest.raises(KeyError):
        with ls.distributed():
            raise KeyError("inside")
    assert all(getattr(dist, name) is obj for name, obj in before.items())
    with pytest.raises(RuntimeError, match="outside run_ranks"):
        ls.get_rank(ls.GROUP)
    with pytest.raises(ValueError):
        ls.get_world_size(None)                                 # only the sentinel group is served


def test_one_rank_runs_at_a_time_and_results_come_back_in_rank_order():
    running, worst = [0], [0]

    def fn(rank):
        assert (ls.get_rank(ls.GROUP), ls.get_world_size(ls.GROUP)) == (rank, 4)
        out = torch.empty(4, 3)
        for _ in range(3):
            running[0] += 1
            worst[0] = max(worst[0], running[0])
            x = torch.full((1, 3), float(rank))
            for _ in range(20):                                 # work that releases the interpreter lock: another rank could get in
                x = x + torch.zeros(1, 3)
            running[0] -= 1
            ls.all_gather_into_tensor(out, x, group=ls.GROUP)
        return rank, threading.current_thread().name, out

    res = ls.run_ranks(4, fn, timeout_s=10.0)
    assert worst[0] == 1
    assert [r[0] for r in res] == [0, 1, 2, 3] and len({r[1] for r in res}) == 4
    assert all(torch.equal(r[2], torch.arange(4.0)[:, None].expand(4, 3)) for r in res)


def test_collectives_and_p2p_move_the_right_blocks():
    def fn(rank):
        G = 3
        src = torch.arange(6.0).view(6, 1) + 10 * rank          # blocks of 2 rows
        out = torch.empty_like(src)
        w = ls.all_to_all_single(out, src, group=ls.GROUP, async_op=True)
        assert w.wait() and ls.all_to_all_single(torch.empty_like(src), src, group=ls.GROUP) is None
        got = torch.empty(2)
        ops = [ls.P2POp(ls.isend, torch.tensor([rank, rank + 0.5]), (rank + 1) % G, group=ls.GROUP),
               ls.P2POp(ls.irecv, got, (rank - 1) % G, group=ls.GROUP)]
        for req in ls.batch_isend_irecv(ops):
            req.wait()
        return out, got

    for rank, (out, got) in enumerate(ls.run_ranks(3, fn, timeout_s=10.0)):
        want = torch.cat([torch.arange(2.0 * rank, 2.0 * rank + 2) + 10 * s for s in range(3)]).view(6, 1)
        assert torch.equal(out, want) and got.tolist() == [(rank - 1) % 3, (rank - 1) % 3 + 0.5]


def _fails_within(world, fn, timeout_s, seconds):
    t0 = time.monotonic()
    with pytest.raises(ls.RankError) as info:
        ls.run_ranks(world, fn, timeout_s=timeout_s)
    assert time.monotonic() - t0 < seconds, "the failure took longer than the timeout allows"
    return info.value


def test_a_rank_that_skips_a_collective_is_an_error_not_a_hang():
    def fn(rank):
        if rank != 1:
            ls.all_gather_into_tensor(torch.empty(3, 2), torch.zeros(1, 2), group=ls.GROUP)

    err = _fails_within(3, fn, 20.0, 5.0)                       # seen when rank 1 returns, long before the timeout
    assert err.rank in (0, 2) and "returned without taking part" in str(err)

    def other_collective(rank):                                 # rank 1 skips the all-to-all and meets the others in the all-gather
        if rank != 1:
            ls.all_to_all_single(torch.empty(2, 2), torch.zeros(2, 2), group=ls.GROUP)
        ls.all_gather_into_tensor(torch.empty(2, 2), torch.zeros(1, 2), group=ls.GROUP)

    err = _fails_within(2, other_collective, 20.0, 5.0)
    assert isinstance(err.__cause__, ValueError) and "disagree" in str(err)


def test_a_receive_without_a_send_is_an_error_not_a_hang():
    def fn(rank):                                               # both wait for a send that never comes: nobody returns, the time runs out
        ls.irecv(torch.empty(2), 1 - rank, group=ls.GROUP).wait()

    err = _fails_within(2, fn, 0.2, 5.0)
    assert isinstance(err.__cause__, TimeoutError) and "receive #0" in str(err)

    def sender_left(rank):
        if rank == 1:
            ls.irecv(torch.empty(2), 0, group=ls.GROUP).wait()

    err = _fails_within(2, sender_left, 20.0, 5.0)
    assert err.rank == 1 and "returned without taking part" in str(err)


def test_leftover_sends_mismatches_and_rank_failures_are_reported():
    def leftover(rank):
        if rank == 0:
            ls.isend(torch.zeros(2), 1, group=ls.GROUP).wait()

    err = _fails_within(2, leftover, 20.0, 5.0)
    assert err.rank is None and "nobody received" in str(err) and "(0, 1, 0)" in str(err)

    def p2p_shape(rank):
        if rank == 0:
            ls.isend(torch.zeros(2), 1, group=ls.GROUP).wait()
        else:
            ls.irecv(torch.zeros(3), 0, group=ls.GROUP).wait()

    err = _fails_within(2, p2p_shape, 20.0, 5.0)
    assert err.rank == 1 and isinstance(err.__cause__, ValueError)

    def p2p_dtype(rank):
        if rank == 0:
            ls.isend(torch.zeros(2), 1, group=ls.GROUP).wait()
        else:
            ls.irecv(torch.zeros(2, dtype=torch.float64), 0, group=ls.GROUP).wait()

    assert isinstance(_fails_within(2, p2p_dtype, 20.0, 5.0).__cause__, ValueError)

    def collective_dtype(rank):
        dt = torch.float32 if rank == 0 else torch.float64
        ls.all_gather_into_tensor(torch.empty(2, 2, dtype=dt), torch.zeros(1, 2, dtype=dt), group=ls.GROUP)

    assert "disagree" in str(_fails_within(2, collective_dtype, 20.0, 5.0))

    def collective_shape(rank):
        ls.all_gather_into_tensor(torch.empty(2, 2 + rank), torch.zeros(1, 2 + rank), group=ls.GROUP)

    assert "disagree" in str(_fails_within(2, collective_shape, 20.0, 5.0))

    def one_rank_raises(rank):
        if rank == 2:
            raise KeyError("rank 2 is broken")
        ls.all_gather_into_tensor(torch.empty(3, 2), torch.zeros(1, 2), group=ls.GROUP)

    err = _fails_within(3, one_rank_raises, 20.0, 5.0)          # the first exception with its rank, not the waiters' PeerFailed
    assert err.rank == 2 and isinstance(err.__cause__, KeyError)


# ------------------------------------------------------- the inputs of tests/test_gpu_parallel_ranks.py, against the oracle alone
import parallel_rank_cases as pc  # noqa: E402


@pytest.mark.parametrize("args", pc.FULL_CASES, ids=pc.case_id)
def test_full_sequence_inputs_meet_their_conditions_and_the_references_tell_mistakes_apart(args):
    pc.check_full_case(pc.full_case(*args))


@pytest.mark.parametrize("kw", pc.RING_CASES, ids=pc.case_id)
def test_ring_inputs_meet_their_conditions_and_the_references_tell_mistakes_apart(kw):
    pc.check_ring_case(pc.ring_case(**kw))
