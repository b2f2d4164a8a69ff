"""Wire-codec kernels of the averaging data plane at the ALBERT-large round sizes: pack and unpack of
one 17.85 M-value tensor, reduce_delta of a reducer's part (V / 8) from k = 8 senders, for FLOAT16
and for BLOCKWISE_8BIT in the same run (the FLOAT16 kernels at equal value count are the yardstick).

    python bench/wire_bench.py [--values 17850000] [--senders 8] [--iters 30] [--out profiles/wire_q8_kernels.jsonl]

Every launch is timed with device events after warm-up, the two codecs alternating launch by launch
and the 256 MB MALL evicted before each; reported per kernel: the median in µs, the 10th and 90th
percentile (the spread to read a difference against) and the effective rate of the bytes the kernel
has to move (fp32 side + wire side, computed from the shapes).  Appends one JSON line to ``--out``."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fns, iters, flush):
    """{name: sorted µs per launch}; the functions take turns, one launch each per round."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    evs = {name: [] for name in fns}
    for _ in range(iters):
        for name, fn in fns.items():
            flush.zero_()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            evs[name].append((a, b))
    torch.cuda.synchronize()
    return {name: sorted(a.elapsed_time(b) * 1e3 for a, b in pairs) for name, pairs in evs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--values", type=int, default=17_850_000)
    ap.add_argument("--senders", type=int, default=8)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wire_q8_kernels.jsonl"))
    args = ap.parse_args()
    assert args.iters >= 20
    if not torch.cuda.is_available():
        raise SystemExit("wire_bench.py measures GPU kernels: no GPU visible")
    import dedloc_amd.ops  # noqa: F401
    from dedloc_amd.ops._lib import q8_bytes

    ops = torch.ops.dedloc
    dev = torch.device("cuda", 0)
    V, k = args.values, args.senders
    P = V // 8
    x = torch.randn(V, device=dev)
    acc = torch.zeros(V, device=dev)
    w16, w8 = torch.empty(V, dtype=torch.float16, device=dev), torch.empty(q8_bytes(V), dtype=torch.uint8, device=dev)
    ops.pack(x, w16, 1.0)
    ops.pack_q8(x, w8)
    weights = torch.rand(k, device=dev) + 0.5
    parts16 = (torch.randn(k, P, device=dev)).half()
    parts8 = torch.empty(k, q8_bytes(P), dtype=torch.uint8, device=dev)
    for i in range(k):
        ops.pack_q8(parts16[i].float(), parts8[i])
    d16, d8 = torch.empty_like(parts16), torch.empty_like(parts8)
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)

    kernels = {  # name: (FLOAT16 launch, its bytes, BLOCKWISE_8BIT launch, its bytes)
        "pack": (lambda: ops.pack(x, w16, 1.0), 4 * V + 2 * V, lambda: ops.pack_q8(x, w8), 4 * V + q8_bytes(V)),
        "reduce_delta": (lambda: ops.reduce_delta(parts16, weights, d16), 2 * k * P * 2,
                         lambda: ops.reduce_delta_q8(parts8, weights, d8, P), 2 * k * q8_bytes(P)),
        "unpack": (lambda: ops.unpack(w16, acc, None, True), 2 * V + 8 * V,
                   lambda: ops.unpack_q8(w8, acc, True), q8_bytes(V) + 8 * V),
    }
    out = {"bench": "wire_q8_kernels", "time": time.time(), "device": torch.cuda.get_device_name(0), "values": V,
           "part_values": P, "senders": k, "iters": args.iters}
    for name, (f16, b16, f8, b8) in kernels.items():
        ts = timed({"FLOAT16": f16, "BLOCKWISE_8BIT": f8}, args.iters, flush)
        for codec, nbytes in (("FLOAT16", b16), ("BLOCKWISE_8BIT", b8)):
            t = ts[codec]
            med = t[len(t) // 2]
            out[f"{name}_{codec}"] = {"us": round(med, 1), "p10_us": round(t[len(t) // 10], 1),
                                      "p90_us": round(t[len(t) * 9 // 10], 1), "bytes": nbytes,
                                      "GBps": round(nbytes / med / 1e3, 1)}
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
