"""Attention kernel micro-benchmark at ALBERT shapes: forward, backward, TFLOP/s.

    python bench/attn_bench.py --batch 64 --heads 16 --seq 512 [--pad 0.25]
    python bench/attn_bench.py --head_dim 128 --impl fused|composed ...

--impl composed runs ops.attn_composed_fwd / _bwd (batched GEMMs + softmax kernel, fp32 scores through
HBM, no tile skipping) on the same inputs: the path every head size outside ops.FUSED_HEAD_DIMS takes.

--varlen [--length_mode full|wikitext|uniform] adds the packed variable-length kernels
(attn_varlen_fwd / _bwd) on rows of those lengths, with TFLOP/s counted on REAL tokens
(sum len^2), beside the fixed-S figures of the same run ("fwd" / "bwd_fused_bias", full rows) and
the fixed-S kernels on the same lengths padded to S ("padded_*", kvinfo lengths, real-token FLOPs).
"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import dedloc_amd.ops as ops  # noqa: E402

O = torch.ops.dedloc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--heads", type=int, default=16)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--pad", type=float, default=0.0, help="fraction of each row that is right padding")
    ap.add_argument("--head_dim", type=int, default=64, choices=(64, 128))
    ap.add_argument("--impl", choices=("fused", "composed"), default="fused")
    ap.add_argument("--varlen", action="store_true", help="also time the packed variable-length kernels")
    ap.add_argument("--length_mode", choices=("full", "wikitext", "uniform"), default="full")
    ap.add_argument("--min_len", type=int, default=64)
    args = ap.parse_args()
    B, H, S, D = args.batch, args.heads, args.seq, args.head_dim
    composed = args.impl == "composed"
    dev = torch.device("cuda")
    qkv = torch.randn(B * S, 3 * H * D, device=dev).bfloat16()
    n = int(round(S * (1 - args.pad)))
    mask = (torch.arange(S, device=dev)[None] < n).expand(B, S).long()
    mbias = torch.where(mask.bool(), 0.0, -1e30).float().contiguous()
    lens = mask.sum(1).int()
    kvinfo = torch.cat([lens, torch.ones(1, dtype=torch.int32, device=dev)]).contiguous()
    scale = 1 / math.sqrt(D)

    def fwd():
        if composed:
            return ops.attn_composed_fwd(qkv, mbias, H, S, scale)
        return O.attn_fwd(qkv, mbias, H, S, scale, kvinfo)

    out, lse = fwd()
    dout = torch.randn_like(out)

    def attn_bwd(db=None):
        if composed:
            return ops.attn_composed_bwd(qkv, mbias, out, dout, lse, H, S, scale, db)
        return O.attn_bwd(qkv, mbias, out, dout, lse, H, S, scale, kvinfo, db)

    def bwd():
        return attn_bwd()

    dbias = torch.zeros(3 * H * D, device=dev)

    def bwd_fused_bias():  # the model's call: QKV bias gradient inside the backward
        return attn_bwd(dbias)

    def bwd_then_colsum():  # the previous form: backward, then a column-sum pass over dqkv
        g = attn_bwd()
        O.bias_grad(g, dbias, True)
        return g

    cases = [("fwd", fwd, 4, B * S * S), ("bwd", bwd, 10, B * S * S), ("bwd_fused_bias", bwd_fused_bias, 10, B * S * S),
             ("bwd_then_colsum", bwd_then_colsum, 10, B * S * S)]
    extra = {}
    if args.varlen:
        from dedloc_amd.data.packing import make_seqinfo
        from dedloc_amd.data.synthetic_mlm import SyntheticSOPStream

        st = SyntheticSOPStream(B, S, 30000, seed=0, length_mode=args.length_mode, min_len=args.min_len)
        vl = st.next_batch()["attention_mask"].sum(1).tolist()
        si, si_h, rows, _ = make_seqinfo(vl, dev, tail=False)
        T = rows[-1]
        vq = torch.randn(T, 3 * H * D, device=dev).bfloat16()
        vout, vlse = O.attn_varlen_fwd(vq, si, si_h, H, scale)
        vdout = torch.randn_like(vout)
        # the fixed-S kernels on the same lengths, padded to S
        pkv = torch.cat([torch.tensor(vl, dtype=torch.int32), torch.ones(1, dtype=torch.int32)]).to(dev)
        pmb = torch.where(torch.arange(S, device=dev)[None] < pkv[:B, None], 0.0, -1e30).float().contiguous()
        pout, plse = O.attn_fwd(qkv, pmb, H, S, scale, pkv)
        real = sum(n * n for n in vl)
        cases += [("varlen_fwd", lambda: O.attn_varlen_fwd(vq, si, si_h, H, scale), 4, real),
                  ("varlen_bwd_fused_bias", lambda: O.attn_varlen_bwd(vq, si, si_h, vout, vdout, vlse, H, scale, dbias),
                   10, real),
                  ("padded_fwd", lambda: O.attn_fwd(qkv, pmb, H, S, scale, pkv), 4, real),
                  ("padded_bwd_fused_bias", lambda: O.attn_bwd(qkv, pmb, pout, dout, plse, H, S, scale, pkv, dbias),
                   10, real)]
        extra = {"length_mode": args.length_mode, "real_token_share": sum(vl) / (B * S), "slot_row_share": T / (B * S)}
    res = {}
    for name, fn, flop_mult, pairs in cases:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(args.iters):
            fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t) / args.iters
        flops = flop_mult * H * pairs * D
        res[name] = {"us": round(dt * 1e6, 1), "tflops": round(flops / dt / 1e12, 1)}
    print(json.dumps({"B": B, "H": H, "S": S, "D": D, "impl": args.impl, "pad": args.pad, **extra, **res}))


if __name__ == "__main__":
    main()
