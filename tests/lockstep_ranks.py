"""G ranks of the multi-GPU drivers in ONE process, one rank at a time (no GPU needed; pinned against gloo by
tests/test_lockstep_ranks_cpu.py, used on the real kernels by tests/test_gpu_parallel_ranks.py).

``run_ranks(world, fn, timeout_s)`` runs ``fn(rank)`` in ``world`` threads. One lock - the baton - lets exactly one rank run at a
time; a rank gives it up only while it waits inside a collective, so a run is deterministic and process-wide state of the drivers
(``flash_attn_interface.fwd_flags`` on the ring's e4m3 path) is never seen half-set by another rank. ``distributed()`` replaces, for
its duration, the names ``liteattention_amd.parallel`` looks up on ``torch.distributed`` (``PATCHED``) by restatements that move data
with ``Tensor.copy_`` on the current stream between the ranks' tensors: collectives in the call (by the last rank to arrive), P2P in the
receive's ``wait()``. All ranks use the same stream, so the order of the data movement is the stream order. The rank comes from a
thread-local, the "process group" is the sentinel ``GROUP``.

P2P is a mailbox keyed by (src, dst, sequence number of that pair): a send posts a REFERENCE to its tensor (read when the receiver
waits; the send's own ``wait()`` does not block, as the grouped sends of ``batch_isend_irecv`` do not), a receive whose send never
comes is a timeout, a send nobody received is an error at the end of ``run_ranks``. Shapes and dtypes must agree between a send and
its receive and between the ranks of one collective. Every wait is bounded by ``timeout_s``; a rank that fails makes every waiting
rank fail, and the caller gets the first exception with its rank (``RankError``). Nothing can hang.

NOT covered: RCCL itself (transport, its own stream, the work handles of ProcessGroupNCCL), real asynchrony between ranks, overlap
timing, and a caller that rewrites a send buffer between ``isend`` and ``wait()``. Those stay with tests/test_gpu_rccl_world1.py (one
real RCCL rank) and an N-GPU node."""
import contextlib
import threading
import time

import torch
import torch.distributed as dist

PATCHED = ("get_world_size", "get_rank", "all_gather_into_tensor", "all_to_all_single", "P2POp", "isend", "irecv",
           "batch_isend_irecv")


class _Group:
    def __repr__(self):
        return "<lockstep process group>"


GROUP = _Group()              # what the drivers get as ``process_group``
_tls = threading.local()      # .ctx (the _World of the run this thread belongs to), .rank


class RankError(RuntimeError):
    """The first failure of a ``run_ranks`` call: ``rank`` (None: the harness itself) and the exception as ``__cause__``."""

    def __init__(self, rank, exc):
        super().__init__(f"rank {rank}: {type(exc).__name__}: {exc}")
        self.rank = rank
        self.__cause__ = exc


class PeerFailed(RuntimeError):
    """Raised in a rank that was waiting when another rank failed."""


class _World:
    def __init__(self, world, timeout_s):
        self.world, self.timeout_s = world, timeout_s
        self.cond = threading.Condition(threading.Lock())      # its lock is the baton
        self.failure = None                                     # (rank, exception) of the first failure
        self.finished = set()                                   # ranks whose fn has returned or raised
        self.n_coll = [0] * world                               # collectives entered, per rank
        self.colls = {}                                         # index -> {"kind", "args": {rank: (out, inp)}, "done"}
        self.mail = {}                                          # (src, dst, seq) -> sent tensor
        self.n_send, self.n_recv = {}, {}                       # (src, dst) -> count

    def fail(self, rank, exc):
        if self.failure is None:
            self.failure = (rank, exc)
        self.cond.notify_all()

    def wait_for(self, ready, peers, what):
        """Give the baton up until ``ready()``; an error once a rank has failed, a rank of ``peers()`` has left, or the time is up."""
        deadline = time.monotonic() + self.timeout_s
        while True:
            if self.failure is not None:
                raise PeerFailed(f"rank {self.failure[0]} failed while this rank waited for {what}")
            if ready():
                return
            gone = sorted(set(peers()) & self.finished)
            if gone:
                raise RuntimeError(f"{what}: rank(s) {gone} returned without taking part")
            left = deadline - time.monotonic()
            if left <= 0:
                raise TimeoutError(f"{what}: not complete after {self.timeout_s} s")
            self.cond.wait(left)


def _ctx(group):
    if group is not GROUP:
        raise ValueError(f"the lockstep collectives serve only lockstep_ranks.GROUP, got group={group!r}")
    ctx = getattr(_tls, "ctx", None)
    if ctx is None:
        raise RuntimeError("a lockstep collective outside run_ranks")
    return ctx, _tls.rank


class _Work:
    """What an asynchronous call returns. ``wait()`` of a collective or a send has nothing left to do; of a receive: see ``_recv``."""

    def __init__(self, on_wait=None):
        self._on_wait, self._done = on_wait, on_wait is None

    def wait(self):
        if not self._done:
            self._on_wait()
            self._done = True
        return True

    def is_completed(self):
        return self._done


def get_world_size(group=None):
    return _ctx(group)[0].world


def get_rank(group=None):
    return _ctx(group)[1]


def _signature(kind, out, inp):
    return (kind, tuple(out.shape), out.dtype, tuple(inp.shape), inp.dtype, out.device, inp.device)


def _collective(kind, out, inp, group, move):
    ctx, rank = _ctx(group)
    idx = ctx.n_coll[rank]
    ctx.n_coll[rank] += 1
    what = f"collective #{idx} ({kind}) of rank {rank}"
    if not out.is_contiguous() or not inp.is_contiguous():
        raise ValueError(f"{what}: both tensors must be contiguous")
    c = ctx.colls.setdefault(idx, {"args": {}, "done": False})
    c["args"][rank] = (kind, out, inp)
    if len(c["args"]) == ctx.world:                 # the last rank to arrive checks and moves everything, on its current stream
        sigs = {r: _signature(*a) for r, a in c["args"].items()}
        if len(set(sigs.values())) != 1:
            raise ValueError(f"collective #{idx}: the ranks disagree on kind / shape / dtype: {sigs}")
        move([c["args"][r][1] for r in range(ctx.world)], [c["args"][r][2] for r in range(ctx.world)])
        c["done"] = True
        del ctx.colls[idx]
        ctx.cond.notify_all()
    else:
        ctx.wait_for(lambda: c["done"], lambda: [r for r in range(ctx.world) if r not in c["args"]], what)
    return _Work()


def all_gather_into_tensor(output_tensor, input_tensor, group=None, async_op=False):
    """Concatenated form (the only one the drivers use): ``output`` is (G * n0, ...) for an input of (n0, ...)."""
    G = _ctx(group)[0].world
    if output_tensor.numel() != G * input_tensor.numel() or output_tensor.dtype != input_tensor.dtype:
        raise ValueError(f"all_gather_into_tensor: output {tuple(output_tensor.shape)} {output_tensor.dtype} does not hold {G} x input "
                         f"{tuple(input_tensor.shape)} {input_tensor.dtype}")

    def move(outs, inps):
        for out in outs:
            flat = out.view(G, -1)
            for src, inp in enumerate(inps):
                flat[src].copy_(inp.view(-1))

    work = _collective("all_gather_into_tensor", output_tensor, input_tensor, group, move)
    return work if async_op else None


def all_to_all_single(output, input, output_split_sizes=None, input_split_sizes=None, group=None, async_op=False):
    """Equal splits along dim 0 (all the drivers use): block ``d`` of rank ``s``'s input becomes block ``s`` of rank ``d``'s output."""
    G = _ctx(group)[0].world
    if output_split_sizes is not None or input_split_sizes is not None:
        raise NotImplementedError("all_to_all_single: equal splits only")
    if tuple(output.shape) != tuple(input.shape) or output.dtype != input.dtype or input.dim() < 1 or input.shape[0] % G:
        raise ValueError(f"all_to_all_single: output {tuple(output.shape)} {output.dtype}, input {tuple(input.shape)} {input.dtype}, "
                         f"{G} ranks: equal shapes and a dim 0 divisible by the number of ranks")

    def move(outs, inps):
        for d, out in enumerate(outs):
            blocks = out.view(G, -1)
            for s, inp in enumerate(inps):
                blocks[s].copy_(inp.view(G, -1)[d])

    work = _collective("all_to_all_single", output, input, group, move)
    return work if async_op else None


def _send(tensor, dst, group):
    ctx, rank = _ctx(group)
    if not 0 <= dst < ctx.world or dst == rank:
        raise ValueError(f"isend of rank {rank}: no such peer {dst}")
    seq = ctx.n_send.get((rank, dst), 0)
    ctx.n_send[(rank, dst)] = seq + 1
    ctx.mail[(rank, dst, seq)] = tensor
    ctx.cond.notify_all()
    return _Work()


def _recv(tensor, src, group):
    ctx, rank = _ctx(group)
    if not 0 <= src < ctx.world or src == rank:
        raise ValueError(f"irecv of rank {rank}: no such peer {src}")
    seq = ctx.n_recv.get((src, rank), 0)
    ctx.n_recv[(src, rank)] = seq + 1
    key = (src, rank, seq)

    def on_wait():
        ctx.wait_for(lambda: key in ctx.mail, lambda: [src], f"receive #{seq} of rank {rank} from rank {src}")
        sent = ctx.mail.pop(key)
        if tuple(sent.shape) != tuple(tensor.shape) or sent.dtype != tensor.dtype:
            raise ValueError(f"receive #{seq} of rank {rank} from rank {src}: sent {tuple(sent.shape)} {sent.dtype}, "
                             f"expected {tuple(tensor.shape)} {tensor.dtype}")
        tensor.copy_(sent)

    return _Work(on_wait)


def isend(tensor, dst=None, group=None, tag=0):
    return _send(tensor, dst, group)


def irecv(tensor, src=None, group=None, tag=0):
    return _recv(tensor, src, group)


class P2POp:
    def __init__(self, op, tensor, peer=None, group=None, tag=0):
        if op is not isend and op is not irecv:
            raise ValueError("P2POp: op must be torch.distributed.isend or torch.distributed.irecv")
        self.op, self.tensor, self.peer, self.group, self.tag = op, tensor, peer, group, tag


def batch_isend_irecv(p2p_op_list):
    if not p2p_op_list or not all(isinstance(op, P2POp) for op in p2p_op_list):
        raise ValueError("batch_isend_irecv: a non-empty list of P2POp")
    return [op.op(op.tensor, op.peer, op.group, op.tag) for op in p2p_op_list]


@contextlib.contextmanager
def distributed():
    """``torch.distributed`` with the names of ``PATCHED`` replaced by this module's; yields the process group to hand to the drivers.
    The originals are put back on the way out, whatever happened inside."""
    here = globals()
    saved = {name: getattr(dist, name) for name in PATCHED}
    try:
        for name in PATCHED:
            setattr(dist, name, here[name])
        yield GROUP
    finally:
        for name, obj in saved.items():
            setattr(dist, name, obj)


def run_ranks(world, fn, timeout_s=30.0):
    """``[fn(0), ..., fn(world - 1)]``, each in a thread of its own, one running at a time (module docstring). Raises ``RankError`` with
    the first failure; a send that nobody received is a failure of the harness's own (rank None)."""
    ctx = _World(world, timeout_s)
    results = [None] * world

    def body(rank):
        with ctx.cond:                               # take the baton
            _tls.ctx, _tls.rank = ctx, rank
            try:
                results[rank] = fn(rank)
            except BaseException as exc:             # noqa: BLE001 - handed to the caller
                ctx.fail(rank, exc)
            finally:
                _tls.ctx = None
                ctx.finished.add(rank)
                ctx.cond.notify_all()

    threads = [threading.Thread(target=body, args=(r,), name=f"lockstep-rank{r}", daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    # every wait inside is bounded by timeout_s and at most `world` of them run out one after another; a rank that is still alive
    # after that is stuck outside any collective
    deadline = time.monotonic() + timeout_s * (world + 1)
    for r, t in enumerate(threads):
        t.join(max(0.0, deadline - time.monotonic()))
        if t.is_alive():
            stuck = TimeoutError(f"rank {r} still running after {timeout_s * (world + 1)} s")
            if ctx.cond.acquire(timeout=1.0):        # not while a rank that never returns holds the baton
                try:
                    ctx.fail(r, stuck)
                finally:
                    ctx.cond.release()
            elif ctx.failure is None:
                ctx.failure = (r, stuck)
            break
    if ctx.failure is None and ctx.mail:
        ctx.failure = (None, RuntimeError(f"sends nobody received (src, dst, sequence number): {sorted(ctx.mail)}"))
    if ctx.failure is not None:
        raise RankError(*ctx.failure)
    return results
