#!/usr/bin/env python
"""kNN evaluation of a SwAV checkpoint (replaces ``swav/vissl/tools/nearest_neighbor_test.py``)::

    python -m dedloc_amd.cli.knn_swav config=pretrain/swav/swav_1node_resnet_submit \\
        +config.CHECKPOINT.PATH=checkpoints/checkpoint.torch \\
        config.DATA.TRAIN.DATA_PATHS='["/data/train"]' \\
        +config.DATA.TEST.DATA_SOURCES=[disk_folder] +config.DATA.TEST.DATA_PATHS='["/data/val"]'

loads a checkpoint written by ``SwavPeer.save_checkpoint``, runs ``training.swav_eval.knn_evaluate``
once with the config's ``NEAREST_NEIGHBOR`` settings (SIGMA, TOPK, FEATURE, MAX_BANK_IMAGES,
MAX_TEST_IMAGES, BANK_PATHS) and prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import sys

from ..utils.config import load_config, parse_cli


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    name, overrides, rest = parse_cli(argv)
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default=None)
    args = ap.parse_args(rest)
    cfg = load_config(name, overrides)
    path = cfg.CHECKPOINT.get("PATH")
    if not path:
        raise SystemExit("knn_swav: +config.CHECKPOINT.PATH=<file written by save_checkpoint> is required")
    import torch

    from ..models.resnet_swav import SwAVModel
    from ..parallel import local_device
    from ..training.swav_eval import build_knn_sets, knn_evaluate_sets

    sets = build_knn_sets(cfg)  # raises before the model is built
    device = local_device(None if args.device is None else torch.device(args.device))
    model = SwAVModel(num_prototypes=int(cfg.MODEL.HEAD.num_clusters),
                      single_pass_every_crop=bool(cfg.MODEL.SINGLE_PASS_EVERY_CROP)).to(device)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    own = model.state_dict()
    with torch.no_grad():
        for k, v in sd["model"].items():
            own[k].copy_(v)
    out = dict(knn_evaluate_sets(model, sets, device), eval=True, checkpoint=str(path),
               iteration=int(sd.get("iteration", -1)), step=int(sd.get("collab_step", -1)))
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
