"""Frozen SwAV trunk: images/s of pooled-feature extraction on synthetic 224x224 bf16 batches, three
arms alternated in one process after a warm-up, timed with HIP events:

  (a) eval       the model's own eval() forward (``SwAVModel.features``: BatchNorm as a broadcast
                 expression after every conv)
  (b) two_kernel the frozen trunk with every BatchNorm as a separate ``bn_apply`` pass
  (c) fused      the frozen trunk with the BatchNorm in the conv's epilogue (``conv2d_bn_act``)
                 wherever conv.hip runs the conv

and, per conv class of the ResNet-50 trunk (stem, the 3x3 of each stage, narrow 1x1, strided 1x1),
the two-kernel form against the fused one on that conv alone.

    python bench/swav_infer_bench.py [--batch 64 256] [--rounds 5] [--iters 3] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CL = torch.channels_last


def _time_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def _alternate(arms, rounds, iters):
    for fn in arms.values():  # warm-up
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            ms[name].append(round(_time_ms(fn, iters), 4))
    return ms


def _median(v):
    return sorted(v)[len(v) // 2]


# (class, Cin, H, Cout, k, stride, pad) at a 224-pixel input: the convs of the trunk that conv.hip runs
CONV_CLASSES = [
    ("stem", 3, 224, 64, 7, 2, 3),
    ("3x3_layer1", 64, 56, 64, 3, 1, 1),
    ("3x3_layer2", 128, 28, 128, 3, 1, 1),
    ("3x3_layer2_s2", 128, 56, 128, 3, 2, 1),
    ("3x3_layer3", 256, 14, 256, 3, 1, 1),
    ("3x3_layer4", 512, 7, 512, 3, 1, 1),
    ("narrow_1x1_layer1", 256, 56, 64, 1, 1, 0),
    ("narrow_1x1_layer2", 512, 28, 128, 1, 1, 0),
    ("strided_1x1_layer2", 256, 56, 512, 1, 2, 0),
    ("strided_1x1_layer4", 1024, 14, 2048, 1, 2, 0),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--class_batch", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import dedloc_amd.ops as dops  # noqa: F401
    from dedloc_amd.models.resnet_swav import SwAVModel

    ops = torch.ops.dedloc
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = SwAVModel().to(dev).eval()
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.running_mean.uniform_(-0.1, 0.1)
                m.running_var.uniform_(0.8, 1.2)
    fused, two = model.frozen_trunk(), model.frozen_trunk(fused=False)
    lines = []
    for b in args.batch:
        x = torch.randn(b, 3, 224, 224, device=dev).bfloat16().contiguous(memory_format=CL)

        def eval_path():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                return model.features(x)

        arms = {"eval": eval_path, "two_kernel": lambda: two(x), "fused": lambda: fused(x)}
        same = bool(torch.equal(fused(x).view(torch.int16), two(x).view(torch.int16)))
        ms = _alternate(arms, args.rounds, args.iters)
        spread_eval = max(ms["eval"]) - min(ms["eval"])
        rec = {"bench": "swav_frozen_trunk", "batch": b, "size": 224, "rounds": args.rounds, "iters": args.iters,
               "ms": ms, "images_per_s": {k: round(b / _median(v) * 1e3, 1) for k, v in ms.items()},
               "eval_spread_ms": round(spread_eval, 4), "fused_equals_two_kernel_bitwise": same,
               "fused_faster_than_eval_outside_spread": max(ms["fused"]) < min(ms["eval"]),
               "fused_faster_than_two_kernel_outside_spread": max(ms["fused"]) < min(ms["two_kernel"])}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del x
    b = args.class_batch
    for name, cin, hw, cout, k, stride, pad in CONV_CLASSES:
        g = torch.Generator(device=dev).manual_seed(cin + cout)
        x = torch.randn(b, cin, hw, hw, device=dev, generator=g).bfloat16().contiguous(memory_format=CL)
        w = (torch.randn(cout, cin, k, k, device=dev, generator=g) / (cin * k * k) ** 0.5).bfloat16()
        w = w.contiguous(memory_format=CL)
        scale = torch.empty(cout, device=dev).uniform_(0.5, 1.5, generator=g)
        shift = torch.randn(cout, device=dev, generator=g)
        zeros, ones = torch.zeros_like(scale), torch.ones_like(scale)
        arms = {"two_kernel": lambda: ops.bn_apply(ops.conv2d_fwd(x, w, stride, pad), None, scale, shift, zeros, ones,
                                                   True, 1),
                "fused": lambda: ops.conv2d_bn_act(x, w, scale, shift, None, True, stride, pad)}
        ms = _alternate(arms, args.rounds, max(args.iters, 10))
        rec = {"bench": "conv2d_bn_act_class", "class": name, "batch": b, "shape": [cin, hw, cout, k, stride, pad],
               "ms": ms, "speedup_median": round(_median(ms["two_kernel"]) / _median(ms["fused"]), 3),
               "fused_faster_outside_spread": max(ms["fused"]) < min(ms["two_kernel"]),
               "fused_slower_outside_spread": min(ms["fused"]) > max(ms["two_kernel"])}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del x, w
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
