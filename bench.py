#!/usr/bin/env python
"""bench.py — headline benchmark of the QK-Skip attention hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W]          (N=1 default)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

Both forms work for N > 1: started WITHOUT a launcher (no RANK / WORLD_SIZE in the environment), ``python bench.py --gpus N``
creates its N ranks itself (`self_launch`: it re-executes this file under torch.distributed.run on 127.0.0.1 with a free port,
one rank per GPU, relays rank 0's JSON line and exits non-zero if any rank failed).

Workload (BASELINE.json metric: "self-attn TFLOPS + ms/step @ seq=75k d=128 bf16, sparsity 0->77%"):
one self-attention call of Wan2.1-14B's video shape — B=1, S=75600, H=40, D=128, bf16 — through
``LiteAttention.__call__`` with an IMPOSED 42 % sparse read list (SURVEY.md §8d "imposed sparsity":
every q-tile keeps the first walked tile plus a contiguous band of (1-s)*Kt key tiles centred on its
diagonal; thr=-inf so the list is a fixed point and every step does identical work). A "step" is one such
call. With N GPUs the 40 heads are sharded (40/N per rank, one skip state per rank, no data-path
collective inside the attention) and the step delivers the all-gathered bf16 output on every rank over RCCL
("scaling": "strong" — total work is fixed). By default (--overlap-windows 3) the attention is issued as 3 launches over
q-tile windows of whole workgroup rounds and the all-gather of window i's rows runs while window i+1 computes
(liteattention_amd/parallel.py); --overlap-windows 1 is the plain "kernel, then one all-gather" step.

`value` = executed TFLOP/s of the whole job = FLOPs of the LISTED tiles (4*rows*cols*D per tile, summed
over all ranks) / step time; skipped tiles are never counted as work. The line also carries the MFMA roofline
of the forward kernel (HIP-event kernel time of the timed steps).

A plain run sets up, runs the W warm-up steps, times the K steps and prints the line; nothing else. With
--full the same line also carries everything measured or checked beside the headline: the sampled-row check
of the timed configuration (`verified`), the power / clock sample, the 1-GPU sparsity sweep (0/21/42/57/77 %:
ms, executed and dense-equivalent TFLOP/s, t(s)/t(0)), the fp8 / other-head-dim / dense / 50-step / half-vote /
text + video sub-records and the CPU baseline (the oracle port timed on the host cores on a bounded sample of
the same workload); the --no-* options switch single parts of --full off.

--dump-outputs DIR writes the output the last timed step returned to its caller (B, S, H, D) as DIR/out.npy in
float32; above 64 MB it is a fixed, seeded sample of whole query rows, whose indices go to DIR/out_rows.npy.
The inputs are seeded, so two builds run with the same arguments can be compared output for output.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_BF16_PEAK_TFLOPS = 2500.0     # dense bf16 MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md
MFMA_FP8_PEAK_TFLOPS = 5000.0      # dense fp8 peak: the block-scaled v_mfma_scale_f32_32x32x64_f8f6f4 the fp8 kernel issues
SPARSITIES = (0.0, 0.21, 0.42, 0.57, 0.77)
HEADLINE_SPARSITY = 0.42


from tools.selfcheck import (banded_rows, executed_flops, impose_lists,  # noqa: E402,F401  (re-exported:
                                         listed_tiles_of_rows, sampled_row_check)          # tools/ and tests import them from here)


def kernel_source_hash() -> str:
    """sha256[:16] over the kernel code (HIP sources, headers and the generated asm bodies): `roofline.traffic` is taken from a
    committed PMC summary only when that summary was measured on exactly this code (a stale byte count is worse than null)."""
    import hashlib
    csrc = os.path.join(ROOT, "liteattention_amd", "csrc")
    h = hashlib.sha256()
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".h", ".inc")):      # .inc = the generated asm bodies (the build writes them)
            with open(os.path.join(csrc, name), "rb") as f:
                h.update(name.encode() + b"\0" + f.read())
    return h.hexdigest()[:16]


def cpu_baseline(S, D, bm, bn, rows, target_seconds=15.0):
    """Time the oracle port (oracle/qkskip_oracle.c, OpenMP) on a bounded sample of the SAME workload:
    one head, the first `n` q-tiles with their 42 % lists against all S keys."""
    from oracle import oracle as orc
    threads = os.cpu_count() or 1
    g = torch.Generator().manual_seed(1)
    k = torch.randn(1, S, 1, D, generator=g).bfloat16()
    v = torch.randn(1, S, 1, D, generator=g).bfloat16()
    k_tiles = -(-S // bn)

    def run(n_qt):
        q = torch.randn(1, n_qt * bm, 1, D, generator=g).bfloat16()
        lists = torch.zeros(2, 1, 1, n_qt, k_tiles + 1, dtype=torch.int32)
        lists[0, 0, 0, :, :5] = rows[:n_qt]
        t0 = time.perf_counter()
        _, _, tiles = orc.qkskip_fwd(q, k, v, block_m=bm, block_n=bn, read_list=lists[0], write_list=lists[1],
                                     thr=float("-inf"))
        dt = time.perf_counter() - t0
        return dt, tiles * 4.0 * bm * bn * D

    dt, fl = run(threads)                       # probe: one q-tile per thread
    n_qt = threads
    for _ in range(3):                          # grow the sample until it is a 10-30 s measurement
        if dt >= 10.0 or n_qt >= rows.shape[0]:
            break
        n_qt = int(min(rows.shape[0], max(n_qt + threads, n_qt * min(8.0, target_seconds / max(dt, 1e-3)))))
        n_qt = max(threads, (n_qt // threads) * threads)
        dt, fl = run(n_qt)
    reps = 1
    while dt < 10.0 and reps < 8:               # many-core hosts finish one head quickly: repeat the sample
        d2, f2 = run(n_qt)
        dt, fl, reps = dt + d2, fl + f2, reps + 1
    res = {"value": round(fl / dt / 1e12, 5), "unit": "TFLOP/s", "cores": threads, "kind": "port",
           "sample": f"{reps} x [1 head x {n_qt} q-tiles ({n_qt * bm} query rows) x all {S} keys at the 42% list], "
                     f"{fl / 1e9:.1f} GFLOP in {dt:.1f} s (oracle/qkskip_oracle.c, OpenMP)"}
    # beside it: the reference's EAGER PyTorch path (attention_ref of hopper/tests/test_util.py:226-348 as restated in
    # oracle.attention_dense_ref: fp32 einsum -> softmax -> einsum) on the same host cores. It has no skip lists: dense,
    # one head, 2048-row query chunks against all S keys (0.6 GB of scores per chunk), a few seconds.
    try:
        torch.set_num_threads(threads)
        chunk, n_chunks, t_e = 2048, 0, 0.0
        qe = torch.randn(1, chunk, 1, D, generator=g).bfloat16()
        orc.attention_dense_ref(qe[:, :256], k, v)                       # warm-up (thread pool, allocator)
        while t_e < 4.0 and n_chunks < 16:
            t0 = time.perf_counter()
            orc.attention_dense_ref(qe, k, v)
            t_e += time.perf_counter() - t0
            n_chunks += 1
        fl_e = 4.0 * chunk * S * D * n_chunks
        res["eager_torch"] = {"value": round(fl_e / t_e / 1e12, 5), "unit": "TFLOP/s (dense)", "cores": threads,
                              "sample": f"{n_chunks} x [1 head x {chunk} query rows x all {S} keys, dense], "
                                        f"{fl_e / 1e9:.1f} GFLOP in {t_e:.1f} s (torch {torch.__version__} CPU eager)"}
    except Exception as e:  # noqa: BLE001
        res["eager_torch"] = {"value": None, "sample": f"failed: {e!r}"}
    return res


def power_sample(launch, n_launches, device_index=0):
    """Socket power and shader clock (rocm-smi) read WHILE `n_launches` queued calls of `launch` keep the GPU busy; outside any timed
    region. The kernels of this path hold the package at its power cap with the clock throttled (HISTORY.md section 4.2): this puts
    the two numbers that say so next to the roofline fraction. Returns None if rocm-smi is not there."""
    import json as _json
    import shutil
    import subprocess
    import torch
    smi = shutil.which("rocm-smi") or "/opt/rocm/bin/rocm-smi"
    if not os.path.exists(smi):
        return None
    for _ in range(n_launches):
        launch()
    time.sleep(0.35)                         # let the power reading settle on the loop
    samples = []
    for _ in range(2):
        try:
            raw = subprocess.run([smi, "-d", str(device_index), "--showpower", "--showclocks", "--showmaxpower", "--json"],
                                 capture_output=True, text=True, timeout=10).stdout
            card = next(iter(_json.loads(raw[raw.index("{"):]).values()))
            samples.append({"socket_w": float(card["Current Socket Graphics Package Power (W)"]),
                            "sclk_mhz": float(card["sclk clock speed:"].strip("()").lower().replace("mhz", "")),
                            "cap_w": float(card["Max Graphics Package Power (W)"])})
        except Exception:  # noqa: BLE001
            pass
    torch.cuda.synchronize()
    if not samples:
        return None
    return {"socket_w": round(sum(x["socket_w"] for x in samples) / len(samples), 1),
            "sclk_mhz": round(sum(x["sclk_mhz"] for x in samples) / len(samples), 1), "cap_w": samples[0]["cap_w"],
            "how": f"rocm-smi, 2 samples while {n_launches} queued launches of the timed configuration run (outside the timed region)"}


# ------------------------------------------------------------------------------------------ creating the ranks
def launched_by_a_launcher(env=None) -> bool:
    """True when a launcher (torch.distributed.run, the driver's N > 1 command) has already created this process as one rank."""
    env = os.environ if env is None else env
    return "RANK" in env and "WORLD_SIZE" in env


def self_launch(argv, n_gpus) -> int:
    """``python bench.py --gpus N`` without a launcher: re-execute this file as N ranks under torch.distributed.run (one process per
    GPU, rendezvous on 127.0.0.1 at a free port). The children's stdout / stderr are this process's own, so rank 0's ONE JSON line
    comes out here; the return code is torchrun's (non-zero when any rank failed)."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, LA_BENCH_SELF_LAUNCHED="1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")         # dmabuf IPC: RCCL between processes fails without it on this driver
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 1) // max(1, n_gpus))))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    return subprocess.run(cmd, env=env).returncode


def load_stand_in():
    """Test seam (tests/test_bench_main_cpu.py): ``LA_BENCH_STANDIN=<module>`` names a module under tests/ whose ``StandIn`` class
    replaces the device (cpu), the collective backend (gloo) and the attention op (a torch restatement that honours the read lists),
    so that THIS file's main() - argument parsing, self-launch, seeding, head partition, agreement, timing, JSON merge, exit codes -
    runs end to end with more than one rank where there is no GPU. The line it prints says so in `data` and is not a measurement."""
    name = os.environ.get("LA_BENCH_STANDIN")
    if not name:
        return None
    import importlib
    return importlib.import_module(name).StandIn()


# ------------------------------------------------------------------------------------------ N > 1 control flow
# Module-level so that a CPU test drives exactly this code with > 2 gloo ranks and a stand-in attention
# (tests/test_distributed_cpu.py::test_bench_multi_gpu_control_flow_world4): no 8-GPU node is available to the builder.
class HostEvent:
    """Stand-in for torch.cuda.Event where there is no device (the gloo test)."""
    def record(self):
        self.t = time.perf_counter()

    def elapsed_time(self, other):
        return (other.t - self.t) * 1e3


def require_world(dist, n_gpus):
    """The line is only valid if the collective backend really spans --gpus ranks: refuse to measure (and to print) otherwise."""
    ws = 1 if dist is None else dist.get_world_size()
    if ws != n_gpus:
        raise SystemExit(f"bench.py: --gpus {n_gpus} but the process group has {ws} rank(s): refusing to print a line "
                         "(launch with torch.distributed.run --nproc-per-node N)")
    return ws


def agree_on_overlapped_form(att, qkv, dist, dev, sync):
    """Decide, on all ranks together, whether the overlapped all-gather is used. A rank that fails AFTER its peers have entered a
    collective cannot be recovered from (the peers wait inside it), so the agreement comes first: every rank runs the windowed
    launches once WITHOUT the collective (``preflight_overlapped``: window planning, the q-tile-window launches, the hook plumbing),
    the verdicts are MIN-all-reduced, and only if every rank passed is one full overlapped step (with its collectives) run as the
    trial. Otherwise ALL ranks fall back to kernel-then-gather. Returns the note for config.overlap_note (None = kept)."""
    ok, note = 1, None
    try:
        att.preflight_overlapped(*qkv)
        sync()
    except Exception as e:  # noqa: BLE001
        ok, note = 0, f"overlapped form failed its local preflight ({e!r}); fell back to one all-gather after the kernel"
    flag = torch.tensor([ok], device=dev, dtype=torch.int32)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if flag.item() == 0:
        att.overlap_windows = 1
        return note or "another rank failed the preflight of the overlapped all-gather; fell back"
    att(*qkv)               # the trial step proper: every rank enters the same collectives
    sync()
    return None


def timed_steps(att, qkv, n_steps, n_warmup, barrier, dist, dev, make_event, keep_last=None):
    """W untimed steps, then exactly K steps between two barriers (+ device sync inside `barrier`); MAX over ranks of the wall time.
    Returns (seconds per step, kernel seconds per step by events on the launch stream). `keep_last`: a list that receives what the
    last timed step returned."""
    for _ in range(n_warmup):
        att(*qkv)
    ev = [(make_event(), make_event()) for _ in range(n_steps)]
    barrier()
    t0 = time.perf_counter()
    for i in range(n_steps - 1):
        att(*qkv, _kernel_events=ev[i])
    out = att(*qkv, _kernel_events=ev[-1])     # only the last result is kept: every step reuses the block its predecessor freed
    barrier()
    if keep_last is not None:
        keep_last.append(out)
    dt = time.perf_counter() - t0
    kern_ms = sum(a.elapsed_time(b) for a, b in ev) / n_steps
    if dist is not None:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = t.item()
    return dt / n_steps, kern_ms / 1e3


DUMP_BYTES = 64 << 20


def dump_outputs(out, dirname, budget=DUMP_BYTES):
    """--dump-outputs: `out` (B, S, H, D), what the last timed step gave its caller, as DIR/out.npy in float32. Above `budget` (3/4 of it
    with headroom for the index file) a fixed sample of whole query rows is written instead: rows drawn by a seed-0 CPU generator, so
    the sample is the same in every run of the same arguments; their indices go to DIR/out_rows.npy (float64)."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    B, S, H, D = out.shape
    for name in ("out.npy", "out_rows.npy"):                      # nothing of an earlier run with other arguments stays beside it
        if os.path.exists(os.path.join(dirname, name)):
            os.remove(os.path.join(dirname, name))
    if out.numel() * 4 <= budget:
        np.save(os.path.join(dirname, "out.npy"), out.float().cpu().numpy())
        return
    n = max(1, min(S, (budget * 3 // 4) // (B * H * D * 4)))
    rows = torch.randperm(S, generator=torch.Generator().manual_seed(0))[:n].sort().values
    sample = out.index_select(1, rows.to(out.device))
    np.save(os.path.join(dirname, "out.npy"), sample.float().cpu().numpy())
    np.save(os.path.join(dirname, "out_rows.npy"), rows.double().numpy())


def multi_gpu_record(dist, dev, kern_s, att, q, out_bytes_per_elem=2):
    """Per-rank kernel time (heads differ in sparsity on real lists; on the imposed lists this shows RCCL interference), the world
    the backend actually sees, each rank's heads, the bytes it sends and receives per step."""
    ws = dist.get_world_size()
    B, S, Hl, D = q.shape
    t = torch.tensor([kern_s * 1e3, float(att.h0), float(att.h1)], device=dev, dtype=torch.float64)
    all_t = [torch.zeros_like(t) for _ in range(ws)]
    dist.all_gather(all_t, t)
    ks = [x[0].item() for x in all_t]
    shard = B * S * Hl * D * out_bytes_per_elem
    return {"rccl_world_size": ws, "backend": dist.get_backend(),
            "kernel_ms_per_rank": [round(x, 3) for x in ks], "kernel_ms_min": round(min(ks), 3), "kernel_ms_max": round(max(ks), 3),
            "heads_per_rank": [[int(x[1].item()), int(x[2].item())] for x in all_t],
            "bytes_sent_per_rank_per_step": (ws - 1) * shard, "bytes_received_per_rank_per_step": (ws - 1) * shard,
            "bytes_gathered_per_rank_per_step": (ws - 1) * shard, "output_shard_bytes": shard,
            "overlapped_form_kept": bool(att.overlap_windows > 1),
            "overlap_windows": len(att.q_windows(q)) if att.overlap_windows > 1 else 1}



def steady_state_ms(launch, est_ms, warm_ms=150.0, timed_ms=300.0, min_reps=5):
    """Median kernel time of `launch` by HIP events on the current stream, in the regime the headline is measured in: the headline loop
    runs 3 warm-up steps of ~50 ms before its 20 timed ones, so a 3-9 ms kernel gets the same ~150 ms of warm-up (the socket is at its
    power cap: the clock a kernel runs at depends on what the GPU did in the last hundred milliseconds; with 2 warm-up launches of a
    4 ms kernel the first timed launches ran 5-7 % slow: tools/debug/dense_sweep.py) and at least `timed_ms` of timed launches."""
    for _ in range(max(2, int(warm_ms / max(est_ms, 0.05)))):
        launch()
    reps = max(min_reps, int(timed_ms / max(est_ms, 0.05)))
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        launch()
        b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev)[reps // 2], reps


def other_head_dims(L, dev, dims=(64, 96, 192, 256), S=16384, H=40):
    """The reference's other default head sizes (hopper/setup.py:57-61), dense bf16 at S=16384 H=40: useful TFLOP/s by HIP events on
    the launch stream (steady state: `steady_state_ms`), and a sampled-row check of the timed output against fp32 torch."""
    import torch
    from tools.selfcheck import sampled_row_check
    out = {"what": f"dense bf16 B=1 S={S} H={H}; per head dim ~150 ms of warm-up launches, then >= 300 ms of timed launches, median", "runs": []}
    g = torch.Generator(device=dev).manual_seed(2)
    for D in dims:
        q, k, v = [torch.randn(1, S, H, D, device=dev, generator=g).bfloat16() for _ in range(3)]
        res = []

        def launch():
            res[:] = L.flash_attn_func(q, k, v, return_softmax_lse=True)
        launch()
        ms, reps = steady_state_ms(launch, est_ms=4.0 * H * S * S * D / 1.2e12)
        o, lse = res
        bm, bn = L.get_tile_sizes(D, 2)
        ver = sampled_row_check(q, k, v, o, lse, None, bm, bn, heads=(0, H - 1), n_rows=64)
        tf = 4.0 * H * S * S * D / (ms * 1e-3) / 1e12
        out["runs"].append({"head_dim": D, "tiles": [bm, bn], "ms": round(ms, 3), "launches_timed": reps, "tflops": round(tf, 1),
                            "frac_of_mfma_peak": round(tf / MFMA_BF16_PEAK_TFLOPS, 4),
                            "verified": {"rows": ver["rows"], "max_err": ver["max_err"], "max_err_lse": ver["max_err_lse"], "ok": ver["ok"]}})
        del q, k, v, o, lse, res
    return out


def fp8_head_dim(L, dev, D, S=16384, H=40):
    """e4m3 at head_dim 64 / 96 / 192 / 256 on the native bodies of round 6 (until then 64 / 96 ran zero-padded on the head_dim-128 body and 192 / 256 on
    the bf16 kernels over up-converted operands), dense at the shape of `other_head_dims`, in the reference's arithmetic (the default) and in
    the two opt-in forms of P; sampled-row check of each timed output (fp8 bounds of the headline fp8 record)."""
    import torch
    from tools.selfcheck import sampled_row_check
    g = torch.Generator(device=dev).manual_seed(4)
    q, k, v = [torch.randn(1, S, H, D, device=dev, generator=g).bfloat16().to(torch.float8_e4m3fn) for _ in range(3)]
    bm, bn = L.get_tile_sizes(D, 1)
    out = {"what": f"dense e4m3 B=1 S={S} H={H} D={D} (V^T prepare pass included); ~150 ms of warm-up launches, then >= 300 ms of timed launches, median",
           "tiles": [bm, bn], "forms": {}}
    for key, env in (("reference_arithmetic", None), ("mfma_rowsum", "mfma_rowsum"), ("encoded_p", "encoded")):
        os.environ.pop("LA_FP8_P", None)
        if env:
            os.environ["LA_FP8_P"] = env
        try:
            res = []

            def launch():
                res[:] = L.flash_attn_func(q, k, v, return_softmax_lse=True)
            launch()
            ms, reps = steady_state_ms(launch, est_ms=4.0 * H * S * S * D / 1.2e12)
            o, lse = res
            ver = sampled_row_check(q, k, v, o, lse, None, bm, bn, heads=(0, H - 1), n_rows=64, o_rtol=0.05, o_atol=1e-3,
                                    lse_atol=2e-4 if env is None else 2.5e-3)
            tf = 4.0 * H * S * S * D / (ms * 1e-3) / 1e12
            out["forms"][key] = {"ms": round(ms, 3), "launches_timed": reps, "tflops": round(tf, 1), "frac_of_mfma_peak": round(tf / MFMA_FP8_PEAK_TFLOPS, 4),
                                 "verified": {"rows": ver["rows"], "max_err": ver["max_err"], "max_err_lse": ver["max_err_lse"], "ok": ver["ok"]}}
        finally:
            os.environ.pop("LA_FP8_P", None)
    return out


def config1_dense(L, dev, S=32768, H=40, D=128):
    """BASELINE.json configs[1]: 1 x MI355X, bf16, seq_len 32768, 40 heads, head_dim 128, 0 % sparsity (dense, FlashAttention-
    equivalent), against the MFMA roofline. Kernel time by HIP events on the launch stream (steady state: `steady_state_ms`);
    sampled-row check of the timed output."""
    g = torch.Generator(device=dev).manual_seed(3)
    q, k, v = [torch.randn(1, S, H, D, device=dev, generator=g).bfloat16() for _ in range(3)]
    res = []

    def launch():
        res[:] = L.flash_attn_func(q, k, v, return_softmax_lse=True)
    launch()
    ms, reps = steady_state_ms(launch, est_ms=4.0 * H * S * S * D / 1.3e12)
    o, lse = res
    bm, bn = L.get_tile_sizes(D, 2)
    ver = sampled_row_check(q, k, v, o, lse, None, bm, bn, heads=(0, H // 2, H - 1), n_rows=128)
    tf = 4.0 * H * S * S * D / (ms * 1e-3) / 1e12
    return {"what": f"configs[1]: dense bf16 B=1 S={S} H={H} D={D}; ~150 ms of warm-up launches, median of {reps} timed launches", "ms": round(ms, 3),
            "tflops": round(tf, 1), "frac_of_mfma_peak": round(tf / MFMA_BF16_PEAK_TFLOPS, 4), "tiles": [bm, bn],
            "verified": {"rows": ver["rows"], "max_err": ver["max_err"], "max_err_lse": ver["max_err_lse"], "ok": ver["ok"]}}


def denoise50(L, dev, thresholds=None, sweep0_ms=None, dense_steps=(5, 15, 25, 35, 45, 49), random_qkv=None, headline_launch=None,
              headline_ms=None, generator="anchored"):
    """BASELINE.json configs[2]. Per threshold: 50 calls of LiteAttention.__call__ on the slowly varying workload; kernel time per
    step by HIP events on the launch stream. Reports the sparsity of the list the LAST step read, its time against the DENSE kernel on
    the same tensors, the 50-step total, and the error the skipping itself introduces at the last step (sparse vs dense kernel
    output; the reference publishes no tolerance for sparse outputs).

    The dense baseline: warmed launches INTERLEAVED with the sparse run - at each of `dense_steps` of every
    threshold's loop the dense kernel runs on that step's tensors, 1 untimed + 3 timed launches, so dense and sparse share the
    thermal state (the order dense / sparse alternates from sampled step to sampled step); a run's t/t_dense uses the median of its own 18 dense samples, `dense_ms_per_step` is the median of all of them,
    and `dense_vs_sweep0` compares it with the dense point of the imposed-list sweep of the same bench run. The sweep runs on random
    q, k, v and the loop on structured ones, which the kernel - at its power limit - does not execute at the same clock; so the dense
    kernel is ALSO timed on the sweep's own random tensors inside the loop (`random_qkv`, one launch pair per sampled step): that number
    against sweep[0] is the like-with-like check of the launch context, the structured-vs-random ratio is the data effect. Measured
    (profiles/r04_bench_line.json): the data does nothing (ratio 0.999) and the CONTEXT does - inside the loop every launch follows
    ~30 ms of memory-bound tensor generation and a host sync, and the same dense launch runs 1.5-5 % slower there than in the
    back-to-back sweep, by box. Sparse and dense are both timed in that context, which is what t / t_dense needs.

    `headline_launch`: the HEADLINE launch itself - the imposed 42 % list on the sweep's random tensors - is timed
    in the same context, one launch per sampled step, and reported as `headline_in_loop` beside the back-to-back `headline_ms`: the
    top-level `ms_per_step` is the cool number, this is the same work inside a pipeline-like loop."""
    from tools.selfcheck import DENOISE_THRESHOLDS, REFERENCE_T_OVER_T0, DenoiseWorkload, lists_to_bitmap, vote_writer_check
    thresholds = DENOISE_THRESHOLDS if thresholds is None else thresholds
    wl = DenoiseWorkload(40, dev, generator=generator)
    ev = lambda: torch.cuda.Event(enable_timing=True)                                           # noqa: E731
    all_dense, all_dense_random, all_headline = [], [], []

    def dense_samples(q, k, v, n=3):
        ref = L.flash_attn_func(q, k, v)                      # untimed: the first launch after another kernel
        evs = [(ev(), ev()) for _ in range(n)]
        for e0, e1 in evs:
            e0.record(); ref = L.flash_attn_func(q, k, v); e1.record()
        torch.cuda.synchronize()
        return [e0.elapsed_time(e1) for e0, e1 in evs], ref

    runs = []
    for name, thr in thresholds:
        att = L.LiteAttention(threshold=thr, max_batch_size=1)
        ms, last_sparsity, dense_ms, ref = [], 0.0, [], None
        for t in range(wl.steps):
            q, k, v = wl.qkv(t)
            last = t == wl.steps - 1
            if last:
                last_sparsity = att.get_skip_fraction(batch=1)
                read49 = att.current_read_list().clone()
            sample = t in dense_steps
            dense_first = sample and (dense_steps.index(t) % 2 == 0)       # alternate the order: neither kernel always runs first after the generation

            def dense_here():
                nonlocal ref, dense_ms
                if random_qkv is not None:
                    all_dense_random.extend(dense_samples(*random_qkv, n=1)[0])
                if headline_launch is not None:
                    headline_launch()                              # untimed: the first launch after another kernel
                    e0, e1 = ev(), ev()
                    e0.record(); headline_launch(); e1.record(); torch.cuda.synchronize()
                    all_headline.append(e0.elapsed_time(e1))
                d_ms, ref = dense_samples(q, k, v)            # at t = 49 `ref` is the dense output the sparse one is compared with
                dense_ms += d_ms
            if dense_first:
                dense_here()
            e0, e1 = ev(), ev()
            e0.record(); out = att(q, k, v, return_softmax_lse=last); e1.record(); torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
            if sample and not dense_first:
                dense_here()
        all_dense += dense_ms
        dense = sorted(dense_ms)[len(dense_ms) // 2]
        out, lse = out
        # the step-49 result against references at full size (tests/test_gpu_denoise_lists.py holds the same checks): sampled rows
        # vs fp32 torch over exactly the keys the READ list names; for sampled (head, q-tile) rows the skip votes and the writer
        # restated in torch vs the row the kernel wrote; no tile the read list skipped reappears in the write list
        try:
            bm, bn = L.get_tile_sizes(128, 2)
            write49 = att.current_read_list()
            ver = sampled_row_check(q, k, v, out, lse, read49, bm, bn, heads=(0, 19, 39), n_rows=128, o_rtol=2.0 ** -7)   # peaked rows: tests/test_gpu_fragmented.py
            gi = torch.Generator().manual_seed(7)
            items = list(zip(torch.randint(0, 40, (16,), generator=gi).tolist(), torch.randint(0, read49.shape[2], (16,), generator=gi).tolist()))
            vw = vote_writer_check(q, k, read49, write49, thr, bm, bn, items)
            subset = int((lists_to_bitmap(write49) & ~lists_to_bitmap(read49)).sum().item()) == 0
            verified = {"ok": bool(ver["ok"] and vw["ok"] and subset), "rows": ver["rows"], "max_err": ver["max_err"], "tol": ver["tol"],
                        "max_err_lse": ver["max_err_lse"], "write_rows_checked": vw["items"], "write_rows_bad": vw["bad"],
                        "write_rows_borderline": vw["borderline"], "max_ranges_in_a_checked_row": vw["max_ranges"],
                        "max_ranges_per_row": int(read49[..., 0].max().item()) // 2, "write_subset_of_read": subset}
            del write49
        except Exception as e:  # noqa: BLE001
            verified = {"ok": False, "error": repr(e)}
        del read49, lse
        d = (out.float() - ref.float()).abs()          # ref = dense kernel on the step-49 tensors
        target = float(name.rstrip("%")) / 100.0 if name.endswith("%") else None
        runs.append({"target": name, "thr": thr, "sparsity_last_step": round(last_sparsity, 4),
                     "within_1pct_of_target": None if target is None else bool(abs(last_sparsity - target) <= 0.01),
                     "ms_last_step": round(ms[-1], 3), "dense_ms_this_run": round(dense, 3), "dense_samples_this_run": len(dense_ms),
                     "t_last_over_dense": round(ms[-1] / dense, 3), "ideal_1_minus_s": round(1 - last_sparsity, 3),
                     "reference_t_over_t0_at_target": REFERENCE_T_OVER_T0.get(name),
                     "total_ms_50_steps": round(sum(ms), 1), "speedup_vs_dense_50_steps": round(dense * wl.steps / sum(ms), 3),
                     "max_abs_err_vs_dense": float(f"{d.max().item():.3e}"), "mean_abs_err_vs_dense": float(f"{d.mean().item():.3e}"),
                     "mean_abs_dense_output": float(f"{ref.float().abs().mean().item():.3e}"), "verified": verified})
        del att, out, d, ref
    dense_all = sorted(all_dense)[len(all_dense) // 2]
    res = {"what": "50 synthetic denoising steps, B=1 S=75600 H=40 D=128 bf16, real skip lists at fixed thresholds "
                   f"(tools.selfcheck.DenoiseWorkload, generator '{generator}'; thresholds bisected for 21 / 42 / 57 / 77 % +- 1 % at "
                   "step 49: " + ("profiles/r04_denoise50_calibration.json)" if generator == "anchored" else
                                  "profiles/r06_denoise50_survey_calibration.json; the generator SURVEY.md 8(d) pins)"),
           "tiles": list(L.get_tile_sizes(128, 2)),
           "dense_ms_per_step": round(dense_all, 3),
           "dense_how": f"median of {len(all_dense)} warmed dense launches interleaved with the sparse runs (steps {list(dense_steps)} of each "
                        "threshold's loop, 1 untimed + 3 timed each)",
           "dense_ms_min_max": [round(min(all_dense), 3), round(max(all_dense), 3)], "runs": runs}
    if all_headline:
        hl = sorted(all_headline)[len(all_headline) // 2]
        res["headline_in_loop"] = {"ms": round(hl, 3), "samples": len(all_headline), "min_max": [round(min(all_headline), 3), round(max(all_headline), 3)],
                                   "back_to_back_kernel_ms": headline_ms, "ratio": None if not headline_ms else round(hl / headline_ms, 4),
                                   "what": "the headline launch (imposed 42 % list, the timed loop's random q / k / v) timed inside the 50-step loop: "
                                           "1 untimed + 1 timed launch at each sampled step, median"}
    if sweep0_ms:
        res["dense_vs_sweep0"] = {"sweep0_kernel_ms": round(sweep0_ms, 3), "ratio": round(dense_all / sweep0_ms, 4),
                                  "note": "sweep[0] = the dense point of the imposed-list sweep (random q, k, v) in this same bench run"}
        if all_dense_random:
            dr = sorted(all_dense_random)[len(all_dense_random) // 2]
            res["dense_vs_sweep0"].update({
                "dense_ms_on_the_sweeps_random_tensors_inside_the_loop": round(dr, 3), "samples": len(all_dense_random),
                "same_tensors_ratio": round(dr / sweep0_ms, 4), "launch_context_effect_pct": round(100.0 * (dr / sweep0_ms - 1.0), 2),
                "structured_over_random_inside_the_loop": round(dense_all / dr, 4),
                "how": "launch_context_effect_pct: the SAME dense launch (the sweep's random tensors) inside the denoising loop against the back-to-back sweep. "
                       "An observation, not a pass / fail: at the power cap a launch that follows ~30 ms of memory-bound tensor generation runs -3...+3 % "
                       "off the back-to-back time, by box and session (both signs were seen); sparse and dense are BOTH timed inside the loop, which is what "
                       "t / t_dense needs. structured_over_random is what the data does to a power-limited kernel"})
        else:
            res["dense_vs_sweep0"]["launch_context_effect_pct"] = round(100.0 * (dense_all / sweep0_ms - 1.0), 2)
    return res


def denoise50_brief(L, dev, thresholds, generator="anchored", env=None):
    """The 50-step run at fixed thresholds without the interleaved dense samples of `denoise50`: per threshold the total kernel time of
    the 50 calls, the last step, the sparsity of the list the last step read, and the error against the DENSE kernel at the last step.
    `env`: environment of the host layer for the run (LA_VOTE=half: the 128-row vote)."""
    from tools.selfcheck import DenoiseWorkload
    saved = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        wl = DenoiseWorkload(40, dev, generator=generator)
        ev = lambda: torch.cuda.Event(enable_timing=True)                                       # noqa: E731
        runs = []
        for name, thr in thresholds:
            att = L.LiteAttention(threshold=thr, max_batch_size=1)
            ms, sp = [], 0.0
            for t in range(wl.steps):
                q, k, v = wl.qkv(t)
                if t == wl.steps - 1:
                    sp = att.get_skip_fraction(batch=1)
                a, b = ev(), ev()
                a.record(); out = att(q, k, v); b.record(); torch.cuda.synchronize()
                ms.append(a.elapsed_time(b))
            ref = L.flash_attn_func(q, k, v)
            d = (out.float() - ref.float()).abs()
            runs.append({"target": name, "thr": thr, "total_ms_50_steps": round(sum(ms), 1), "ms_last_step": round(ms[-1], 3),
                         "sparsity_last_step": round(sp, 4), "mean_abs_err_vs_dense": float(f"{d.mean().item():.3e}"),
                         "max_abs_err_vs_dense": float(f"{d.max().item():.3e}")})
            del att, out, ref, d
        return {"tiles": list(L.get_tile_sizes(128, 2)), "generator": generator, "runs": runs}
    finally:
        for k, v_ in saved.items():
            if v_ is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v_


def half_vote_record(L, dev, qkv, tile_runs, S=75600, H=40, D=128):
    """LA_FLAG_HALF_VOTE (skip lists per 128-row half of the 256-row workgroup; LA_VOTE=half) beside the default 256-row vote, same box, same
    process: (1) the imposed lists at 42 % and 77 % in the 128-row geometry - at a given SPARSITY the form may cost nothing (the union walk of
    two banded halves is two tiles longer); (2) the 50-step run at the SAME FIXED thresholds as `denoise50` - a 128-row vote drops more
    tiles at a threshold, and the error against the dense kernel says what that costs."""
    from tools.selfcheck import DENOISE_THRESHOLDS
    q, k, v = qkv
    os.environ["LA_VOTE"] = "half"
    try:
        bm, bn = L.get_tile_sizes(D, 2)
        qt, kt = -(-S // bm), -(-S // bn)
        att = L.LiteAttention(threshold=-10.0, max_batch_size=1)
        att.threshold = float("-inf")
        att._get_read_write_lists(q, k)
        att._phase = 0
        imposed = []
        for s_ in (0.42, 0.77):
            rows = banded_rows(qt, kt, bm, bn, s_)
            impose_lists(att, rows)
            ms, reps = steady_state_ms(lambda: att(q, k, v), est_ms=50.0, min_reps=8)
            fl = executed_flops(rows, H, 1, S, S, bm, bn, D)
            imposed.append({"sparsity": round(1 - listed_tiles_of_rows(rows) / (qt * kt), 4), "ms": round(ms, 3), "executed_tflops": round(fl / ms / 1e9, 1),
                            "frac_of_mfma_peak": round(fl / ms / 1e9 / MFMA_BF16_PEAK_TFLOPS, 4)})
        del att
    finally:
        os.environ.pop("LA_VOTE", None)
    brief = denoise50_brief(L, dev, DENOISE_THRESHOLDS, env={"LA_VOTE": "half"})
    ratio = {}
    for r in brief["runs"]:
        base = next((x for x in tile_runs if x["target"] == r["target"]), None)
        if base:
            ratio[r["target"]] = {"thr": r["thr"], "total_ms_half_over_tile256": round(r["total_ms_50_steps"] / base["total_ms_50_steps"], 4),
                                  "sparsity_last_step": [base["sparsity_last_step"], r["sparsity_last_step"]],
                                  "mean_abs_err_vs_dense": [base["mean_abs_err_vs_dense"], r["mean_abs_err_vs_dense"]]}
    return {"what": "LA_FLAG_HALF_VOTE (LA_VOTE=half): lists per 128-row half, tiles (128, 64); pairs are [256-row vote, 128-row vote]",
            "imposed_lists": imposed, "denoise50": brief, "at_fixed_thresholds": ratio}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seqlen", type=int, default=75600)
    ap.add_argument("--heads", type=int, default=40)
    ap.add_argument("--full", action="store_true",
                    help="besides the headline, run every check and sub-record of the line (sampled-row check, power sample, sparsity sweep, "
                         "fp8, other head dims, dense S=32768, 50-step runs, half vote, text + video recipe, CPU baseline); off: the plain "
                         "run sets up, warms up, times the steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned as DIR/out.npy (float32; a fixed, seeded sample "
                         "of whole query rows above 64 MB, their indices in DIR/out_rows.npy)")
    ap.add_argument("--no-sweep", action="store_true", help="--full: skip the 1-GPU sparsity sweep")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-fp8", action="store_true", help="--full: skip the fp8 (configs[4]) sub-record of the 1-GPU bf16 line")
    ap.add_argument("--no-verify", action="store_true", help="--full: skip the sampled-row check after the timed loop")
    ap.add_argument("--no-power", action="store_true", help="--full: skip the rocm-smi power / clock sample")
    ap.add_argument("--no-head-dims", action="store_true", help="--full: skip the head_dim 64 / 96 / 192 / 256 sub-record of the 1-GPU bf16 line")
    ap.add_argument("--no-denoise", action="store_true", help="--full: skip the 50-step denoising run (BASELINE.json configs[2]) of the 1-GPU bf16 line")
    ap.add_argument("--prewarm-steps", type=int, default=0,
                    help="untimed steps of the timed configuration BEFORE the W warm-up steps (outside the contract's warm-up and timed region): the socket is at "
                         "its power cap and the clock the first steps after start-up run at is 1-3 %% below the sustained one (round 5: the 20 steps after 3 warm-ups "
                         "51.0 ms, the same configuration a few seconds later in the same process 50.4 ms); 0 = off (the default since round 6: the contract's --warmup W alone "
                         "governs the state that is timed)")
    ap.add_argument("--overlap-windows", type=int, default=3,
                    help="N > 1: q-tile windows per step whose all-gathers overlap the next window's compute (1 = off)")
    ap.add_argument("--dtype", choices=["bf16", "fp16", "fp8"], default="bf16",
                    help="bf16 = headline (BASELINE.json configs[2,3]); fp8 = configs[4] (e4m3 Q/K/V, bf16 out)")
    args = ap.parse_args()
    full = args.full

    # LA_BENCH_FORCE_DIST=1: run the N > 1 code path (process group, trial step, overlapped all-gather, agreement
    # all-reduce) on ONE rank too - a 1-rank RCCL all-gather is a copy on RCCL's stream. For exercising this file on a 1-GPU box.
    want_dist = args.gpus > 1 or os.environ.get("LA_BENCH_FORCE_DIST") == "1"
    if want_dist and not launched_by_a_launcher():
        sys.exit(self_launch(sys.argv[1:], args.gpus))           # the N ranks are created here; each of them re-enters main()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher created WORLD_SIZE={world} rank(s): no line is printed for a "
                         "world other than --gpus (start it as `python bench.py --gpus N`, or under torch.distributed.run "
                         "--nproc-per-node N)")
    seam = load_stand_in()
    if seam is None:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a GPU (no CPU fallback in the product path)")
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
        backend, device_sync, new_event = "nccl", torch.cuda.synchronize, (lambda: torch.cuda.Event(enable_timing=True))
    else:
        dev, backend, device_sync, new_event = torch.device("cpu"), "gloo", (lambda: None), HostEvent
    dist = None
    force_dist = os.environ.get("LA_BENCH_FORCE_DIST") == "1" and "MASTER_ADDR" in os.environ
    if world > 1 or force_dist:
        import torch.distributed as dist_mod
        dist = dist_mod
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if seam is None:
            dist.init_process_group(backend=backend, device_id=dev)
        else:
            dist.init_process_group(backend=backend)
    require_world(dist, args.gpus)

    import liteattention_amd as L
    from liteattention_amd.parallel import HeadShardedLiteAttention

    B, S, H, D = 1, args.seqlen, args.heads, 128
    assert H % world == 0, "heads must divide over ranks"
    Hl = H // world

    g = torch.Generator(device=dev).manual_seed(1234 + rank)         # every rank draws ITS heads: no broadcast, no shared tensor
    qkv_bf16 = [torch.randn(B, S, Hl, D, device=dev, generator=g, dtype=torch.float32).to(torch.bfloat16) for _ in range(3)]

    def barrier():
        if dist is not None:
            dist.barrier()
        device_sync()

    def run_dtype(dtype_name, steps, warmup, sweep, distributed, keep_last=None):
        """Headline measurement (+ with --full: verification, power sample, optional sparsity sweep) for one input dtype on this rank's
        heads. `keep_last`: a list that receives what the last timed step returned."""
        fp8 = dtype_name == "fp8"
        peak = MFMA_FP8_PEAK_TFLOPS if fp8 else MFMA_BF16_PEAK_TFLOPS
        q, k, v = [x.to(torch.float8_e4m3fn) for x in qkv_bf16] if fp8 else ([x.half() for x in qkv_bf16] if dtype_name == "fp16" else qkv_bf16)
        bm, bn = L.get_tile_sizes(D, 1 if fp8 else 2)
        q_tiles, k_tiles = -(-S // bm), -(-S // bn)
        use_dist = dist if distributed else None
        att = HeadShardedLiteAttention(num_heads=H, threshold=-10.0, max_batch_size=B,
                                       process_group=None if use_dist is None else dist.group.WORLD,
                                       overlap_windows=args.overlap_windows if use_dist is not None else 1,
                                       _collective_at_world_1=force_dist, **({} if seam is None else seam.attention_kwargs()))
        att.local.threshold = float("-inf")     # imposed lists are a fixed point: identical work every step
        if seam is not None:
            seam.bind(att, bm, bn)
        local_call = (lambda: att.local(q, k, v, return_softmax_lse=True)) if seam is None else (lambda: seam.local_call(q, k, v))

        def set_sparsity(s):
            rows = banded_rows(q_tiles, k_tiles, bm, bn, s)
            if att.local._skip_list is None:
                att.local._get_read_write_lists(q, k)          # allocate for this shape
                att.local._phase = 0
            impose_lists(att.local, rows)
            return rows

        def timed(n_steps, n_warmup, keep_last=None):
            return timed_steps(att, (q, k, v), n_steps, n_warmup, barrier, use_dist, dev, new_event, keep_last)

        # ---- headline: 42 % imposed sparsity
        rows = set_sparsity(HEADLINE_SPARSITY)
        overlap_note = None
        if use_dist is not None and att.overlap_windows > 1:
            overlap_note = agree_on_overlapped_form(att, (q, k, v), dist, dev, device_sync)
        flops_rank = executed_flops(rows, Hl, B, S, S, bm, bn, D)
        for _ in range(max(0, args.prewarm_steps)):          # the same number on every rank (the step may hold a collective)
            att(q, k, v)
        step_s, kern_s = timed(steps, warmup, keep_last)
        flops_job = flops_rank * world
        listed_frac = listed_tiles_of_rows(rows) / (q_tiles * k_tiles)
        kernel_name = ("la_prep_v_fp8_kernel + la_fwd_x64_fp8_kernel<true>" if fp8 else
                       f"la_fwd_x64_kernel<true, {'true' if dtype_name == 'fp16' else 'false'}, 128>")   # <SKIPABLE, F16, D>
        # algorithmic minimum HBM bytes of one launch: Q + K + V once at the input width, O once in bf16 (lists and LSE are <2 %)
        esz = 1 if fp8 else 2
        alg_bytes = B * S * Hl * D * (3 * esz + 2)
        res = {
            "value": round(flops_job / step_s / 1e12, 2),
            "ms_per_step": round(step_s * 1e3, 3),
            "tiles": [bm, bn], "sparsity": round(1 - listed_frac, 4),
            "dense_equiv_tflops": round(4.0 * B * H * S * S * D / step_s / 1e12, 2),
            "roofline": {"bound": "mfma", "achieved": round(flops_rank / kern_s / 1e12, 2), "peak": peak, "unit": "TFLOP/s",
                         "frac": round(flops_rank / kern_s / 1e12 / peak, 4), "traffic": None, "kernel": kernel_name,
                         "kernel_ms": round(kern_s * 1e3, 3),
                         "algorithmic_tflop_per_launch": round(flops_rank / 1e12, 3),
                         "algorithmic_hbm_bytes_per_launch": alg_bytes},
            "overlap_note": overlap_note,
            "parallelism": f"heads sharded {world}x{Hl}" + (
                "" if use_dist is None else
                (f" + RCCL all-gather of O in {len(att.q_windows(q))} q-tile windows overlapped with compute"
                 if att.overlap_windows > 1 else " + 1 RCCL all-gather of O per step")),
        }
        # traffic: only from a PMC summary measured on exactly these kernel sources
        pmc = os.path.join(ROOT, "profiles", {"fp8": "pmc_summary_fp8.json", "fp16": "pmc_summary_fp16.json"}.get(dtype_name, "pmc_summary.json"))
        if os.path.exists(pmc):
            try:
                with open(pmc) as f:
                    p = json.load(f)
                if p.get("kernel_source_sha16") == kernel_source_hash() and p.get("n_gpus", 1) == world:
                    res["roofline"]["traffic"] = p.get("hbm_bytes_per_launch")
                    res["roofline"]["traffic_source"] = p.get("source")
                else:
                    res["roofline"]["traffic_source"] = "none: profiles/" + os.path.basename(pmc) + " was measured on other kernel sources"
            except Exception:
                pass

        if use_dist is not None:
            res["multi_gpu"] = multi_gpu_record(dist, dev, kern_s, att, q)

        # ---- correctness gate on the timed configuration: sampled rows vs an fp32 torch reference with the same block mask
        if full and not args.no_verify:
            try:
                rows42 = set_sparsity(HEADLINE_SPARSITY)
                read_list = att.local._skip_list[att.local._phase].clone()
                out, lse = local_call()
                heads = sorted({0, Hl // 2, Hl - 1})
                lse8 = 2e-4 if os.environ.get("LA_FP8_P", "") in ("", "reference") else 2.5e-3      # fp8 LSE by form of P: tests/test_gpu_headline.py
                tol = dict(o_rtol=0.05, o_atol=1e-3, lse_atol=lse8) if fp8 else dict(o_rtol=2.0 ** -8, o_atol=1e-4)
                ver = sampled_row_check(q, k, v, out, lse, read_list, bm, bn, heads, n_rows=256, **tol)
                ver["finite"] = bool(torch.isfinite(out.float()).all().item())
                ver["lists_fixed_point"] = bool(torch.equal(att.local._skip_list[0], att.local._skip_list[1]))
                ver["ok"] = bool(ver["ok"] and ver["finite"] and ver["lists_fixed_point"])
                ver["what"] = (f"{ver['rows']} query rows ({len(heads)} heads x 256) of the timed {HEADLINE_SPARSITY:.0%} configuration vs fp32 "
                               "torch attention over the listed keys; whole output finite; write list == read list at thr=-inf")
                del out, lse
            except Exception as e:  # noqa: BLE001
                ver = {"ok": False, "error": repr(e)}
            if use_dist is not None:
                flag = torch.tensor([1 if ver.get("ok") else 0], device=dev, dtype=torch.int32)
                dist.all_reduce(flag, op=dist.ReduceOp.MIN)
                ver["ok_all_ranks"] = bool(flag.item())
                ver["ok"] = bool(ver.get("ok") and ver["ok_all_ranks"])
            res["verified"] = ver

        # ---- package power / clock under the timed configuration (1 GPU only; about a second)
        if full and use_dist is None and seam is None and not args.no_power:
            try:
                set_sparsity(HEADLINE_SPARSITY)
                n_q = max(8, int(1.2 / max(step_s, 1e-4)))
                pw = power_sample(lambda: att(q, k, v), n_q, dev.index or 0)
                if pw is not None:
                    res["power"] = pw
            except Exception:  # noqa: BLE001
                pass

        # ---- 1-GPU sparsity sweep (the reference's sparsity-vs-runtime curve, README.md:81-87)
        if sweep:
            sw = []
            for s_ in SPARSITIES:
                r = set_sparsity(s_)
                fl = executed_flops(r, Hl, B, S, S, bm, bn, D)
                st, ks_ = timed(max(5, steps // 2), 2)
                sw.append({"sparsity": round(1 - listed_tiles_of_rows(r) / (q_tiles * k_tiles), 4),
                           "ms": round(st * 1e3, 3), "kernel_ms": round(ks_ * 1e3, 3),
                           "executed_tflops": round(fl / st / 1e12, 1),
                           "dense_equiv_tflops": round(4.0 * B * H * S * S * D / st / 1e12, 1)})
            t0 = sw[0]["ms"]
            ref_curve = {0.0: 1.0, 0.21: 0.824, 0.42: 0.601, 0.57: 0.443, 0.77: 0.235}
            for e, s_ in zip(sw, SPARSITIES):
                e["t_over_t0"] = round(e["ms"] / t0, 3)
                e["reference_t_over_t0"] = ref_curve[s_]
            res["sweep"] = sw
        res["_bm_bn_tiles"] = (bm, bn, q_tiles, k_tiles)

        def headline_again():
            set_sparsity(HEADLINE_SPARSITY)
            return lambda: att(q, k, v)
        res["_headline_again"] = headline_again
        return res

    # (the stand-in seam of the CPU tests has no device: the 1-GPU sub-records - sweep, fp8, head dims, 50-step run, CPU baseline - stay out of its line)
    last = []
    main_res = run_dtype(args.dtype, args.steps, args.warmup, sweep=(full and world == 1 and seam is None and not args.no_sweep), distributed=True,
                         keep_last=last)
    bm, bn, q_tiles, k_tiles = main_res.pop("_bm_bn_tiles")
    headline_again = main_res.pop("_headline_again")
    if args.dump_outputs and rank == 0:
        out = last[0] if isinstance(last[0], torch.Tensor) and last[0].dim() == 4 else HeadShardedLiteAttention.to_bshd(last[0])
        dump_outputs(out, args.dump_outputs)
        del out
    del last

    result = {
        "metric": "self-attn TFLOPS + ms/step @ seq=75k d=128 bf16, sparsity 0->77%; 1/2/4/8 GPU",
        "value": main_res["value"],
        "unit": "TFLOP/s (executed: FLOPs of listed tiles only)",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "prewarm_steps": max(0, args.prewarm_steps),
        "ms_per_step": main_res["ms_per_step"],
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": args.dtype, "data": "synthetic" if seam is None else "STAND-IN attention on the CPU over gloo (test seam): NOT a measurement",
        "config": {"workload": f"QK-Skip self-attention fwd, B={B} S={S} H={H} D={D} {args.dtype}, imposed "
                               f"{HEADLINE_SPARSITY:.0%} sparsity (banded lists, thr=-inf), tiles {bm}x{bn}",
                   "sparsity": main_res["sparsity"],
                   "parallelism": main_res["parallelism"],
                   "launcher": ("self-launched: python bench.py --gpus N re-executed itself under torch.distributed.run"
                                if os.environ.get("LA_BENCH_SELF_LAUNCHED") == "1" else
                                ("external launcher (torch.distributed.run)" if launched_by_a_launcher() else "single process")),
                   "dense_equiv_tflops": main_res["dense_equiv_tflops"]},
        "roofline": main_res["roofline"],
    }
    if main_res.get("overlap_note"):
        result["config"]["overlap_note"] = main_res["overlap_note"]
    for key in ("verified", "multi_gpu", "power", "sweep"):
        if key in main_res:
            result[key] = main_res[key]

    # ---- BASELINE.json configs[4] beside the headline: the same workload with e4m3 Q/K/V (bf16 out), a few extra seconds
    if full and world == 1 and seam is None and args.dtype == "bf16" and not args.no_fp8:
        try:
            f8 = run_dtype("fp8", max(5, args.steps // 2), 2, sweep=False, distributed=False)
            f8.pop("_bm_bn_tiles"); f8.pop("_headline_again")
            result["fp8"] = {"value": f8["value"], "unit": result["unit"], "ms_per_step": f8["ms_per_step"], "dtype": "fp8 (e4m3 in, fp32 accumulate, bf16 out)",
                             "steps": max(5, args.steps // 2), "sparsity": f8["sparsity"], "tiles": f8["tiles"],
                             "roofline": f8["roofline"], "verified": f8.get("verified"), "power": f8.get("power"),
                             "p_form": "default = the reference's arithmetic: P by v_exp_f32 + hardware e4m3 rounding (softmax.h:85-87), fp32 row sums of the "
                                       "un-rounded P on the vector unit (softmax.h:275-296)"}
            result["fp8"]["p_form_of_value"] = "reference_arithmetic (the default since round 6)"
            # beside it, on the same lists and the same box, the two opt-in forms that trade the reference's arithmetic for throughput:
            #   mfma_rowsum = LA_FLAG_FP8_MFMA_ROWSUM: the reference's P, row sums of the ROUNDED P from the matrix pipe
            #   encoded_p   = LA_FLAG_FP8_ENCODED_P: the block-scaled log-linear e4m3 encoding of P (include/lite_attention_amd.h) - NOT the reference's arithmetic
            for key, val in (("mfma_rowsum", "mfma_rowsum"), ("encoded_p", "encoded")):
                os.environ["LA_FP8_P"] = val
                try:
                    fx = run_dtype("fp8", max(5, args.steps // 2), 2, sweep=False, distributed=False)
                    result["fp8"][key] = {"value": fx["value"], "ms_per_step": fx["ms_per_step"], "frac": fx["roofline"]["frac"],
                                          "verified": {k: fx.get("verified", {}).get(k) for k in ("ok", "max_err", "max_err_lse", "tol")}}
                finally:
                    os.environ.pop("LA_FP8_P", None)
            result["fp8"]["reference_arithmetic"] = "value (the default form)"
            if not args.no_head_dims:
                for hd in (64, 96, 192, 256):
                    result["fp8"][f"head_dim_{hd}"] = fp8_head_dim(L, dev, hd)
        except Exception as e:  # noqa: BLE001
            result["fp8"] = {"value": None, "error": repr(e)}

    # ---- BASELINE.json configs[1]: dense S=32768 H=40 (well under a second)
    if full and world == 1 and seam is None and args.dtype == "bf16" and not args.no_head_dims:
        try:
            result["config1_dense_s32768"] = config1_dense(L, dev)
        except Exception as e:  # noqa: BLE001
            result["config1_dense_s32768"] = {"error": repr(e)}

    # ---- the reference's other default head sizes beside the headline 128 (about a second)
    if full and world == 1 and seam is None and args.dtype == "bf16" and not args.no_head_dims:
        try:
            result["other_head_dims"] = other_head_dims(L, dev)
        except Exception as e:  # noqa: BLE001
            result["other_head_dims"] = {"error": repr(e)}

    # ---- BASELINE.json configs[2]: 50 synthetic denoising steps with REAL (fragmented, per-head) skip lists at fixed thresholds
    # (selfcheck.DENOISE_THRESHOLDS: bisected on all 40 heads for 21 / 42 / 57 / 77 % +- 1 % last-step sparsity, tools/calibrate_denoise.py)
    if full and world == 1 and seam is None and args.dtype == "bf16" and not args.no_denoise and S == 75600 and H == 40:
        try:
            sw0 = result.get("sweep", [{}])[0].get("kernel_ms")
            result["denoise50"] = denoise50(L, dev, sweep0_ms=sw0, random_qkv=qkv_bf16 if world == 1 else None,
                                            headline_launch=headline_again(), headline_ms=main_res["roofline"]["kernel_ms"])
            hil = result["denoise50"].get("headline_in_loop")
            if hil:                                    # beside the cool number, at the top level
                result["ms_per_step_in_denoise_loop"] = hil["ms"]
        except Exception as e:  # noqa: BLE001
            result["denoise50"] = {"error": repr(e)}

    # ---- round 6 sub-records: the 128-row vote beside the default, the generator SURVEY.md 8(d) pins, the reference's text + video recipe
    extra = full and world == 1 and seam is None and args.dtype == "bf16" and S == 75600 and H == 40
    if extra and not args.no_denoise and "runs" in result.get("denoise50", {}):
        try:
            result["half_vote"] = half_vote_record(L, dev, qkv_bf16, result["denoise50"]["runs"])
        except Exception as e:  # noqa: BLE001
            result["half_vote"] = {"error": repr(e)}
        try:
            from tools.selfcheck import SURVEY_DENOISE_THRESHOLDS
            result["denoise50_survey"] = denoise50_brief(L, dev, SURVEY_DENOISE_THRESHOLDS, generator="survey")
        except Exception as e:  # noqa: BLE001
            result["denoise50_survey"] = {"error": repr(e)}
    if extra and not args.no_head_dims:
        try:
            from tools.joint_recipe_bench import joint_recipe
            result["joint_recipe"] = joint_recipe(L, dev, qkv_bf16)
        except Exception as e:  # noqa: BLE001
            result["joint_recipe"] = {"error": repr(e)}
    # ---- the numbers of the sub-records that are meant to be read, where the driver keeps them: roofline / config
    try:
        rf, cf = result["roofline"], result["config"]
        if "sweep" in result:
            cf["t_over_t0"] = [e["t_over_t0"] for e in result["sweep"]]
            cf["reference_t_over_t0"] = [e["reference_t_over_t0"] for e in result["sweep"]]
            cf["sweep_sparsities"] = [e["sparsity"] for e in result["sweep"]]
        if result.get("fp8", {}).get("roofline"):
            rf["fp8_reference_frac"] = result["fp8"]["roofline"]["frac"]          # the default fp8 form = the reference's arithmetic
            for key in ("mfma_rowsum", "encoded_p"):
                if key in result["fp8"]:
                    rf[f"fp8_{key}_frac"] = result["fp8"][key]["frac"]
            for hd in (64, 96, 192, 256):
                if "forms" in result["fp8"].get(f"head_dim_{hd}", {}):
                    rf[f"fp8_head_dim_{hd}_frac"] = {k: f["frac_of_mfma_peak"] for k, f in result["fp8"][f"head_dim_{hd}"]["forms"].items()}
        if "runs" in result.get("other_head_dims", {}):
            rf["other_head_dims"] = {str(r["head_dim"]): r["frac_of_mfma_peak"] for r in result["other_head_dims"]["runs"]}
        if "frac_of_mfma_peak" in result.get("config1_dense_s32768", {}):
            rf["config1_dense_s32768_frac"] = result["config1_dense_s32768"]["frac_of_mfma_peak"]
        if "runs" in result.get("denoise50", {}):
            cf["denoise50_total_ms"] = {r["target"]: r["total_ms_50_steps"] for r in result["denoise50"]["runs"]}
            cf["denoise50_t_last_over_dense"] = {r["target"]: r["t_last_over_dense"] for r in result["denoise50"]["runs"]}
        if "at_fixed_thresholds" in result.get("half_vote", {}):
            cf["half_vote_total_ms_over_tile256"] = {k_: v_["total_ms_half_over_tile256"] for k_, v_ in result["half_vote"]["at_fixed_thresholds"].items()}
            cf["half_vote_imposed_ms"] = {str(e["sparsity"]): e["ms"] for e in result["half_vote"]["imposed_lists"]}
        if "runs" in result.get("denoise50_survey", {}):
            cf["denoise50_survey_total_ms"] = {r["target"]: [r["thr"], r["sparsity_last_step"], r["total_ms_50_steps"]] for r in result["denoise50_survey"]["runs"]}
        if "everything_but_v2v_over_v2v" in result.get("joint_recipe", {}):
            cf["joint_recipe_small_calls_over_v2v"] = result["joint_recipe"]["everything_but_v2v_over_v2v"]
            rf["joint_recipe_frac"] = {n: result["joint_recipe"][n]["frac_of_mfma_peak"] for n in ("t2t", "t2v", "v2t", "v2v")}
    except Exception as e:  # noqa: BLE001
        result["summary_keys_error"] = repr(e)

    if full and world == 1 and seam is None and rank == 0 and not args.no_cpu_baseline and args.dtype == "bf16":
        try:
            result["cpu_baseline"] = cpu_baseline(S, D, bm, bn, banded_rows(q_tiles, k_tiles, bm, bn, HEADLINE_SPARSITY))
        except Exception as e:  # the baseline is a reported number, never the measured path
            result["cpu_baseline"] = {"value": None, "unit": "TFLOP/s", "cores": os.cpu_count(), "kind": "port",
                                      "sample": f"failed: {e!r}"}

    if rank == 0:
        print(json.dumps(result))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
