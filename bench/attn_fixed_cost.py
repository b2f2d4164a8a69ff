"""Fixed per-workgroup cost of the three head_dim-64 attention kernels.

    python bench/attn_fixed_cost.py --out profiles/attn_fixed_cost.jsonl --tag before

Times attn_fwd / attn_bwd_dq / attn_bwd_dkdv (the model's calls: key lengths, fused bias gradient)
at S = 128, 256, 512 with B * S = 262144 tokens and H = 16, i.e. 2, 4 and 8 tile iterations per
workgroup, from a rocprofv3 kernel trace of this script's own --run mode (one process per S).  With
n workgroups of k tiles each, kernel time / n = a * k + c: a least-squares line through the three
points gives a (time per tile iteration) and c (the per-workgroup intercept: operand staging, ring
fill, normalise / store, lse, bias-gradient tail), both in ns of kernel time per workgroup, i.e.
already divided by however many workgroups the device runs side by side.  `fixed_share_s512` is
c / (8 a + c).  Appends one JSON line per kernel to --out.
--seqs 512 only prints the three kernels' median times at that length (the per-kernel figure of an
A/B run with DEDLOC_NATIVE_LIB).
"""
import argparse
import csv
import glob
import json
import math
import os
import statistics
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TOKENS, H, D = 262144, 16, 64
SEQS = (128, 256, 512)
# kernel-name fragment -> rows (queries or keys) per workgroup
KERNELS = {"attn_fwd_kernel": 256, "attn_bwd_dq_kernel": 256, "attn_bwd_dkdv_kernel": 128}


def run(S, iters):
    import torch

    import dedloc_amd.ops  # noqa: F401

    O = torch.ops.dedloc
    B = TOKENS // S
    dev = torch.device("cuda")
    qkv = torch.randn(B * S, 3 * H * D, device=dev).bfloat16()
    mbias = torch.zeros(B, S, device=dev)
    kvinfo = torch.cat([torch.full((B,), S, dtype=torch.int32), torch.ones(1, dtype=torch.int32)]).to(dev)
    scale = 1 / math.sqrt(D)
    dbias = torch.zeros(3 * H * D, device=dev)
    out, lse = O.attn_fwd(qkv, mbias, H, S, scale, kvinfo)
    dout = torch.randn_like(out)
    for _ in range(iters + 2):  # the first two calls of each kernel are dropped as warm-up
        O.attn_fwd(qkv, mbias, H, S, scale, kvinfo)
        O.attn_bwd(qkv, mbias, out, dout, lse, H, S, scale, kvinfo, dbias)
    torch.cuda.synchronize()


def trace(S, iters, timeout):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "p", "--", sys.executable,
               os.path.abspath(__file__), "--run", str(S), "--iters", str(iters)]
        subprocess.run(cmd, check=True, timeout=timeout, stdout=subprocess.DEVNULL)
        dur = {k: [] for k in KERNELS}
        for path in glob.glob(os.path.join(d, "**", "*_kernel_trace.csv"), recursive=True):
            rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
            for r in rows:
                for k in KERNELS:
                    if k in r["Kernel_Name"]:
                        dur[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: statistics.median(v[3:]) for k, v in dur.items()}  # [3:]: the priming call and two warm-ups


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", type=int, default=0, help="(internal) run the kernels at this S and exit")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="")
    ap.add_argument("--timeout", type=float, default=150)
    ap.add_argument("--seqs", default=None, help="comma list instead of 128,256,512: times only, no line fit")
    args = ap.parse_args()
    if args.run:
        run(args.run, args.iters)
        return
    if args.seqs:  # per-kernel times at the given lengths (A/B of one kernel), no fit
        for S in (int(x) for x in args.seqs.split(",")):
            t = trace(S, args.iters, args.timeout)
            print(json.dumps({"tag": args.tag, "S": S, **{k: round(v, 1) for k, v in t.items()}}), flush=True)
        return
    us = {S: trace(S, args.iters, args.timeout) for S in SEQS}
    for k, rows in KERNELS.items():
        pts = []
        for S in SEQS:
            n_wg = (TOKENS // S) * H * ((S + rows - 1) // rows)
            pts.append((S // 64, us[S][k] * 1e3 / n_wg))
        mx, my = sum(p[0] for p in pts) / 3, sum(p[1] for p in pts) / 3
        a = sum((x - mx) * (y - my) for x, y in pts) / sum((x - mx) ** 2 for x, _ in pts)
        c = my - a * mx
        rec = {"tag": args.tag, "kernel": k, "us": {str(S): round(us[S][k], 1) for S in SEQS},
               "ns_per_wg": {str(64 * x): round(y, 2) for x, y in pts}, "ns_per_tile": round(a, 3),
               "ns_fixed_per_wg": round(c, 3), "fixed_share_s512": round(c / (8 * a + c), 4)}
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
