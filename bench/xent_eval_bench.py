"""Evaluation cross-entropy (xent_eval: one read of the logits) against the training kernel
(xent_fwd_bwd: two reads, one write) on the same [M, V] bf16 logits: µs per call, cold cache, back
to back in one process, and the HBM rate of the bytes each call must move.

    python bench/xent_eval_bench.py [--M 4096] [--V 30000 31995] [--iters 30]

Prints one JSON line per V (timing loop of bench/ln_bench.py)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench.ln_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=4096)
    ap.add_argument("--V", type=int, nargs="+", default=[30000, 31995])
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    import dedloc_amd.ops as dops

    ops = torch.ops.dedloc
    for V in args.V:
        M = args.M
        x = (torch.randn(M, V, device="cuda") * 3).bfloat16()
        lab = torch.randint(0, V, (M,), device="cuda")
        lab[::7] = -100
        e = M * V * 2
        out = {"M": M, "V": V, "aligned_rows": V % 8 == 0}
        t = timed(lambda: ops.xent_eval(x, lab, -100), args.iters)
        out["xent_eval_us"], out["xent_eval_TBps"] = round(t, 1), round(e / t / 1e6, 3)
        t = timed(lambda: dops.eval_cross_entropy(x, lab), args.iters)  # + the per-row reductions
        out["eval_cross_entropy_us"] = round(t, 1)
        t = timed(lambda: ops.xent_fwd_bwd(x, lab, False, -100), args.iters)
        out["xent_fwd_bwd_us"], out["xent_fwd_bwd_TBps"] = round(t, 1), round(3 * e / t / 1e6, 3)
        # a one-read streaming pass over the same bytes on this box
        t = timed(lambda: torch.amax(x, dim=1), args.iters)
        out["amax_us"], out["amax_TBps"] = round(t, 1), round(e / t / 1e6, 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
