"""The MLM head's decoder + loss alone, forward and backward: the fused kernels
(ops.mlm_cross_entropy) against the composed path (ops.linear then ops.cross_entropy) on the same
inputs, at the headline micro-batch's M = 39424 target rows and V = 30000.

    python bench/mlm_head_bench.py [--M 39424] [--V 30000] [--rounds 3] [--iters 10] [--out FILE]
                                   [--splits N ...]

The arms alternate call by call inside each round (device events around one forward + backward,
cold MALL, median of --iters after a warm-up of every arm); one JSON line per round with the time
per call and ``max_memory_allocated`` of each arm above the bytes held before it ran, appended to
--out (default profiles/mlm_xent.jsonl).

    python bench/mlm_head_bench.py --eval [--M 32768] ...

times the evaluation instead, forward only: ops.mlm_eval_cross_entropy against the decoder GEMM
(ops.linear) + ops.eval_cross_entropy that evaluate_batch ran before it, at the evaluation batch's
M = 64 x 512 rows (--M 4928 for 64 x 77); the same record with each arm's loss sum and top-1 / top-5
counts, appended to profiles/mlm_eval.jsonl.

``fused`` is the launcher's own choice of vocabulary slices (``splits=0``).  --splits adds one arm
``fused_s{n}`` per forced slice count to the same alternation: ``--splits 1`` is the unsplit kernels,
a longer list is the sweep the launcher's rule in csrc/kernels/mlm_xent.hip is set from
(profiles/mlm_head_split.jsonl)."""
import argparse
import functools
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--eval", action="store_true", help="the evaluation arms (forward only)")
    ap.add_argument("--M", type=int, default=None, help="rows (default 39424; --eval: 32768)")
    ap.add_argument("--V", type=int, default=30000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--splits", type=int, nargs="*", default=[], help="forced vocabulary slice counts, one arm each")
    args = ap.parse_args()
    args.M = args.M or (32768 if args.eval else 39424)
    args.out = args.out or os.path.join(ROOT, "profiles", "mlm_eval.jsonl" if args.eval else "mlm_xent.jsonl")
    if not torch.cuda.is_available():
        raise SystemExit("mlm_head_bench needs a GPU")
    import dedloc_amd.ops as ops

    M, V = args.M, args.V
    g = torch.Generator().manual_seed(0)
    t = torch.randn(M, 128, generator=g).bfloat16().cuda().requires_grad_()
    w = (torch.randn(V, 128, generator=g) * 0.5).bfloat16().cuda()
    bias = (torch.randn(V, generator=g) * 0.1).bfloat16().cuda()
    labels = torch.randint(0, V, (M,), generator=g).cuda()
    gw = torch.zeros(V, 128, device="cuda")
    gb = torch.zeros(V, device="cuda")
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")  # evicts the 256 MB MALL

    def fused(splits=0):
        return ops.mlm_cross_entropy(t, w, bias, labels, gw, gb, splits=splits)

    def composed():
        return ops.cross_entropy(ops.linear(t, w, bias, gw, gb), labels)

    def fused_eval(splits=0):
        return ops.mlm_eval_cross_entropy(t, w, bias, labels, splits=splits)

    def composed_eval():
        return ops.eval_cross_entropy(ops.linear(t, w, bias), labels)

    arms = {"fused": fused_eval, "composed": composed_eval} if args.eval else {"fused": fused, "composed": composed}
    for n in args.splits:
        arms[f"fused_s{n}"] = functools.partial(fused_eval if args.eval else fused, n)
    stats = {}

    def call(fn):
        if args.eval:
            with torch.no_grad():
                out = fn()
            stats[fn] = {k: v for k, v in out.items() if k != "loss_sum"}
            return out["loss_sum"]
        t.grad = None
        loss = fn()
        loss.backward()
        return loss

    peak = {}
    for name, fn in arms.items():  # warm-up of both arms, and each arm's peak memory on its own
        call(fn)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        loss = call(fn)
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
        peak[name + "_loss"] = float(loss)
        peak[name + "_stats"] = {k: int(v) for k, v in stats.get(fn, {}).items()}
        del loss
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for rnd in range(args.rounds):
        evs = {name: [] for name in arms}
        for _ in range(args.iters):
            for name, fn in arms.items():
                flush.zero_()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call(fn)
                b.record()
                evs[name].append((a, b))
        torch.cuda.synchronize()
        rec = {"bench": "mlm_eval" if args.eval else "mlm_head", "M": M, "V": V, "round": rnd, "iters": args.iters,
               "logits_bytes": M * V * 2}
        for name in arms:
            ts = sorted(a.elapsed_time(b) * 1e3 for a, b in evs[name])
            rec[name + "_us"] = round(ts[len(ts) // 2], 1)
            rec[name + "_peak_bytes"] = peak[name]
            rec[name + "_loss"] = peak[name + "_loss"]
            rec.update({f"{name}_{k}": v for k, v in peak[name + "_stats"].items()})
        rec["peak_drop_bytes"] = peak["composed"] - peak["fused"]
        print(json.dumps(rec), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
