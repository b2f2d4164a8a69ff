"""The fused evaluation pool (ops.avgpool_bn_stats: pool + BatchNorm statistics, x read once) against
the same result composed from stock torch ops on the same tensor (NCHW view of the channels-last
activation -> avg_pool2d -> var_mean), at the five default taps of LINEAR_EVAL.PROTOCOL=eval_mlp.

    python bench/avgpool_bn_stats_bench.py [--batch 256] [--size 224] [--reps 20] [--out FILE]

The arms alternate call by call; between calls a 512 MiB buffer is overwritten so neither arm finds
its input in the 256 MiB last-level cache.  Times are device events around one call (the fused
arm's two kernels; the stock arm's kernels), medians over ``--reps``.  ``x_TBps`` is the bytes of x,
counted once, over the fused median.  ``copy_TBps`` is a same-session device-to-device copy of a
buffer of x's size, counted read + write (bench/hip/bw_probe.hip is the standalone roof probe).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, flush):
    flush()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import dedloc_amd.ops as ops
    from dedloc_amd.training.swav_linear import DEFAULT_POOLS, TAPS, tap_shapes

    dev = torch.device("cuda", 0)
    scrub = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    flush = lambda: scrub.fill_(1)  # noqa: E731
    lines = []
    for tap in TAPS:
        C, H, W = tap_shapes(args.size)[tap]
        k, s, p = DEFAULT_POOLS[tap]
        x = (torch.randn(args.batch, C, H, W, device=dev) * 2 + 0.5).bfloat16().contiguous(memory_format=torch.channels_last)
        dst = torch.empty_like(x)

        def fused():
            return ops.avgpool_bn_stats(x, k, s, p)

        def stock():
            y = torch.nn.functional.avg_pool2d(x, k, s, p)
            return y, torch.var_mean(y.float(), dim=(0, 2, 3), unbiased=False)

        for _ in range(3):
            fused(), stock(), dst.copy_(x)
        t = {"fused": [], "stock": [], "copy": []}
        for _ in range(args.reps):
            for name, fn in (("fused", fused), ("stock", stock), ("copy", lambda: dst.copy_(x))):
                t[name].append(_timed(fn, flush)[0])
        yf, s1, _ = fused()
        ys, (var, mean) = stock()
        R = yf.numel() // C
        agree = ((s1 / R - mean).abs().max() / mean.abs().max()).item()
        nbytes = x.numel() * 2
        med = {n: statistics.median(v) for n, v in t.items()}
        line = {"bench": "avgpool_bn_stats", "tap": tap, "batch": args.batch, "shape": [C, H, W], "pool": [k, s, p],
                "x_MB": round(nbytes / 1e6, 1), "fused_us": round(med["fused"] * 1e6, 1),
                "stock_us": round(med["stock"] * 1e6, 1), "fused_min_us": round(min(t["fused"]) * 1e6, 1),
                "stock_min_us": round(min(t["stock"]) * 1e6, 1), "x_TBps": round(nbytes / med["fused"] / 1e12, 3),
                "copy_us": round(med["copy"] * 1e6, 1), "copy_TBps": round(2 * nbytes / med["copy"] / 1e12, 3),
                "speedup": round(med["stock"] / med["fused"], 2), "mean_rel_diff_vs_stock": agree, "reps": args.reps}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del x, dst
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
