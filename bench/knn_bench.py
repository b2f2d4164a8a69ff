"""kNN evaluation: the fused similarity + top-k kernel (dedloc::knn_topk) against the composed route
the reference takes (a [chunk, N] fp32 score matrix per 512-row query chunk through dedloc::bmm,
then torch.topk), and the feature extraction of the same number of images for scale.

    python bench/knn_bench.py [--Q 4096] [--N 131072] [--k 200] [--D 128 2048] [--rounds 3] [--iters 3]
                              [--feature_images 4096] [--out profiles/knn_eval.jsonl]

Both arms run alternated in one process, ``rounds`` rounds of ``iters`` calls each after a warm-up,
timed with HIP events; one JSON line per D (ms per call and round, and whether the fused kernel is
faster outside the spread of the rounds) and one for ``extract_features``."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def composed_topk(q, bank, k, chunk=512):
    """The reference's route (nearest_neighbor_test.py): scores of one query chunk in memory, topk."""
    ops = torch.ops.dedloc
    bt = bank.t().unsqueeze(0)
    vals, idx = [], []
    for r0 in range(0, q.shape[0], chunk):
        s = ops.bmm(q[r0:r0 + chunk].unsqueeze(0), bt, True)[0]
        v, i = torch.topk(s, k, dim=1, largest=True, sorted=True)
        vals.append(v)
        idx.append(i)
    return torch.cat(vals), torch.cat(idx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Q", type=int, default=4096)
    ap.add_argument("--N", type=int, default=131072)
    ap.add_argument("--k", type=int, default=200)
    ap.add_argument("--D", type=int, nargs="+", default=[128, 2048])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--splits", type=int, default=0)
    ap.add_argument("--feature_images", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import dedloc_amd.ops as dops  # noqa: F401

    ops = torch.ops.dedloc
    dev = torch.device("cuda", 0)
    lines = []
    for D in args.D:
        g = torch.Generator(device=dev).manual_seed(D)
        q = torch.nn.functional.normalize(torch.randn(args.Q, D, device=dev, generator=g)).bfloat16()
        bank = torch.nn.functional.normalize(torch.randn(args.N, D, device=dev, generator=g)).bfloat16()
        arms = {"fused": lambda: ops.knn_topk(q, bank, args.k, args.splits),
                "composed": lambda: composed_topk(q, bank, args.k)}
        fv, fi = arms["fused"]()
        cv, ci = arms["composed"]()
        # same neighbours up to the order of fp32-equal scores (the composed route has no tie rule)
        agree = float((fi.long() == ci).float().mean())
        for fn in arms.values():  # warm-up
            fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in arms}
        for _ in range(args.rounds):
            for name, fn in arms.items():
                ms[name].append(round(_time_ms(fn, args.iters), 3))
        rec = {"bench": "knn_topk", "Q": args.Q, "N": args.N, "k": args.k, "D": D, "splits": args.splits,
               "fused_ms": ms["fused"], "composed_ms": ms["composed"], "index_agreement": round(agree, 6),
               "max_val_diff": float((fv - cv).abs().max()),
               "fused_faster_outside_spread": max(ms["fused"]) < min(ms["composed"]),
               "speedup_median": round(sorted(ms["composed"])[len(ms["composed"]) // 2]
                                       / sorted(ms["fused"])[len(ms["fused"]) // 2], 3)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del q, bank, fv, fi, cv, ci
    if args.feature_images > 0:
        from dedloc_amd.models.resnet_swav import SwAVModel
        from dedloc_amd.training.swav_eval import extract_features

        torch.manual_seed(0)
        model = SwAVModel().to(dev)
        b = 64
        x = torch.randn(b, 3, 224, 224, device=dev).bfloat16().contiguous(memory_format=torch.channels_last)
        y = torch.zeros(b, dtype=torch.int64, device=dev)
        batches = [(x, y)] * (args.feature_images // b)
        extract_features(model, batches[:2])  # warm-up
        torch.cuda.synchronize()
        t = [round(_time_ms(lambda: extract_features(model, batches), 1), 1) for _ in range(2)]
        rec = {"bench": "extract_features", "images": b * len(batches), "batch": b, "size": 224, "feature": "trunk",
               "ms": t, "note": "model forward only (device-resident batches, no decode)"}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
