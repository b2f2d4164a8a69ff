"""Wall time of one linear-evaluation training epoch (training/swav_linear.py) over a folder of
pre-decoded ``.npy`` images, and of its three phases on their own: the data stream (decode threads,
packing, host-to-device copy, the ragged random-resized-crop sampler), the frozen-trunk forward and
the head's step.  The phases overlap in the real epoch (the stream decodes ahead, the GPU work is
asynchronous), so the epoch is bounded by the slowest of them, not by their sum.

    python bench/swav_linear_epoch.py [--images 10000] [--batch 256] [--classes 10] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _folder(root, images, classes, seed=0):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (400, 400, 3), dtype=np.uint8)
    for k in range(images):
        d = os.path.join(root, f"class{k % classes:03d}")
        os.makedirs(d, exist_ok=True)
        h, w = int(rng.integers(180, 321)), int(rng.integers(180, 321))
        i, j = int(rng.integers(0, 400 - h + 1)), int(rng.integers(0, 400 - w + 1))
        np.save(os.path.join(d, f"{k}.npy"), np.ascontiguousarray(base[i:i + h, j:j + w]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import dedloc_amd.ops as dops  # noqa: F401
    from dedloc_amd.data.image_folder import ImageFolderDataset, ImageFolderLabelledStream
    from dedloc_amd.models.resnet_swav import SwAVModel
    from dedloc_amd.training.swav_linear import LinearProbe, train_linear

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = SwAVModel().to(dev)
    trunk = model.frozen_trunk()
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        _folder(root, args.images, args.classes)
        gen_s = time.perf_counter() - t0
        ds = ImageFolderDataset([root])

        def stream():
            return ImageFolderLabelledStream(ds, args.batch, dev, num_workers=args.workers)

        s = stream()
        steps = s.steps_per_epoch()
        x = y = None
        for xb, yb in s.epoch(0):  # warm-up: page cache, pinned buffers, kernels
            trunk(xb)
            if x is None:
                x, y = xb, yb  # a full batch (the epoch's last one is short)
        f = trunk(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in s.epoch(1):
            pass
        torch.cuda.synchronize()
        data_s = time.perf_counter() - t0
        probe = LinearProbe(args.classes, device=dev)
        probe.train_step(f, y, 0.0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            f = trunk(x)
        torch.cuda.synchronize()
        fwd_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        for _ in range(steps):
            probe.train_step(f, y, 0.0)
        torch.cuda.synchronize()
        head_s = time.perf_counter() - t0
        s.close()

        class _Short:  # one test batch: the epoch under measure is the training epoch
            def __iter__(self):
                yield x, y

        s = stream()
        t0 = time.perf_counter()
        train_linear(trunk, s, _Short(), args.classes, dict(NUM_EPOCHS=1, BATCH_SIZE=args.batch), dev)
        torch.cuda.synchronize()
        epoch_s = time.perf_counter() - t0
        s.close()
    phases = {"data": data_s, "forward": fwd_s, "head": head_s}
    out = {"bench": "swav_linear_epoch", "images": args.images, "batch": args.batch, "classes": args.classes,
           "steps": steps, "workers": args.workers, "epoch_s": round(epoch_s, 3),
           "images_per_s": round(args.images / epoch_s, 1), "phase_s": {k: round(v, 3) for k, v in phases.items()},
           "bound_by": max(phases, key=phases.get), "folder_generation_s": round(gen_s, 1),
           "note": ".npy images of 180-320 px a side (no JPEG decode); forward and head timed on full batches"}
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
