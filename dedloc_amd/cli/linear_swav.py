#!/usr/bin/env python
"""Linear evaluation of a SwAV checkpoint (the reference's
``benchmark/linear_image_classification/imagenet1k/other_styles/
eval_resnet_res5_avgpool_output_8gpu_transfer_in1k_linear`` protocol)::

    python -m dedloc_amd.cli.linear_swav config=pretrain/swav/swav_1node_resnet_submit \\
        +config.CHECKPOINT.PATH=checkpoints/checkpoint.torch \\
        config.DATA.TRAIN.DATA_SOURCES=[disk_folder] +config.DATA.TRAIN.DATA_PATHS='["/data/train"]' \\
        +config.DATA.TEST.DATA_SOURCES=[disk_folder] +config.DATA.TEST.DATA_PATHS='["/data/val"]'

loads a checkpoint written by ``SwavPeer.save_checkpoint``, trains one linear layer on the frozen
trunk's pooled features (``training.swav_linear``) with the config's ``LINEAR_EVAL`` settings
(NUM_EPOCHS, BATCH_SIZE, TEST_EVERY_NUM_EPOCH, MAX_TRAIN_IMAGES, MAX_TEST_IMAGES, CROP_SIZE, RESIZE,
CENTER_CROP, BASE_LR, SCHEDULE, VALUES, MILESTONES, ...), appends one JSON line per evaluation to
``METRICS_FILE`` and prints the final one.
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
        raise SystemExit("linear_swav: +config.CHECKPOINT.PATH=<file written by save_checkpoint> is required")
    import torch

    from ..models.resnet_swav import SwAVModel
    from ..parallel import local_device
    from ..training.swav_linear import build_linear_sets, linear_evaluate

    sets = build_linear_sets(cfg)  # raises before the model is built
    device = local_device(None if args.device is None else torch.device(args.device))
    model = SwAVModel(num_prototypes=int(cfg.MODEL.HEAD.num_clusters),
                      single_pass_every_crop=bool(cfg.MODEL.SINGLE_PASS_EVERY_CROP)).to(device)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    own = model.state_dict()
    with torch.no_grad():
        for k, v in sd["model"].items():
            own[k].copy_(v)
    extra = dict(checkpoint=str(path), iteration=int(sd.get("iteration", -1)), step=int(sd.get("collab_step", -1)))
    out = linear_evaluate(model, sets, device, cfg.get("METRICS_FILE"), extra)[-1]
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
