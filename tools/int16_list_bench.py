"""Headline launch with int32 and with int16 skip lists, side by side.

The launch bench.py times - ``LiteAttention.__call__`` at B = 1, S = 75 600, H = 40, head_dim 128, bf16, the IMPOSED 42 % banded list
(tools/selfcheck.py, a fixed point under thr = -inf) - with the same warm-up and step counts (3 / 20), measured by HIP events around
every call, once per list element type and alternating between the two so that clock drift hits both. The list element type cannot
change the arithmetic; this shows whether it changes the time (the rows are read once per item by one wave: 2.4 or 4.7 KB out of the
~20 MB of K / V an item streams).

    python tools/int16_list_bench.py [--rounds 3] [--steps 20] [--warmup 3] [--seqlen 75600] [--heads 40] [--vote half]

Prints one JSON line: per element type the per-round mean kernel ms, their mean, and the ratio int16 / int32."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seqlen", type=int, default=75600)
    ap.add_argument("--heads", type=int, default=40)
    ap.add_argument("--sparsity", type=float, default=0.42)
    ap.add_argument("--vote", choices=["default", "half"], default="default")
    args = ap.parse_args()
    if args.vote == "half":
        os.environ["LA_VOTE"] = "half"
    import liteattention_amd as L
    from selfcheck import banded_rows, executed_flops, impose_lists

    B, S, H, D = 1, args.seqlen, args.heads, 128
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    q, k, v = [torch.randn(B, S, H, D, device=dev, generator=g).bfloat16() for _ in range(3)]
    bm, bn = L.get_tile_sizes(D, 2)
    rows = banded_rows(-(-S // bm), -(-S // bn), bm, bn, args.sparsity)
    flops = executed_flops(rows, H, B, S, S, bm, bn, D)
    atts, outs = {}, {}
    for name, dt in (("int32", torch.int32), ("int16", torch.int16)):
        att = L.LiteAttention(threshold=-10.0, max_batch_size=B, list_dtype=dt)
        att.threshold = float("-inf")
        att._get_read_write_lists(q, k)
        att._phase = 0
        impose_lists(att, rows)
        atts[name] = att
        outs[name] = att(q, k, v, return_softmax_lse=True)
    torch.cuda.synchronize()
    same = torch.equal(outs["int32"][0], outs["int16"][0]) and torch.equal(outs["int32"][1], outs["int16"][1])
    ms = {"int32": [], "int16": []}
    for _ in range(args.rounds):
        for name in ("int32", "int16"):
            att = atts[name]
            for _ in range(args.warmup):
                att(q, k, v)
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
            for a, b in ev:
                a.record()
                att(q, k, v)
                b.record()
            torch.cuda.synchronize()
            ms[name].append(sum(a.elapsed_time(b) for a, b in ev) / args.steps)
    mean = {n: sum(x) / len(x) for n, x in ms.items()}
    print(json.dumps({
        "workload": f"B={B} S={S} H={H} D={D} bf16, imposed {args.sparsity:.0%} list, vote={args.vote}, tiles=({bm}, {bn})",
        "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "results_bit_identical": same,
        "list_bytes": {n: atts[n]._skip_list.nbytes for n in atts},
        "ms_per_round": {n: [round(x, 3) for x in xs] for n, xs in ms.items()},
        "ms_mean": {n: round(x, 3) for n, x in mean.items()},
        "tflops": {n: round(flops / x / 1e9, 1) for n, x in mean.items()},
        "int16_over_int32": round(mean["int16"] / mean["int32"], 4),
    }))


if __name__ == "__main__":
    main()
