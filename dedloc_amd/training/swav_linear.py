"""Linear evaluation of a SwAV model: one linear classifier trained on the frozen trunk's pooled
``res5`` features — SwAV's published quality metric, the reference's
``configs/config/benchmark/linear_image_classification/imagenet1k/other_styles/
eval_resnet_res5_avgpool_output_8gpu_transfer_in1k_linear.yaml``.

The trunk runs as ``SwAVModel.frozen_trunk()`` (a snapshot: BatchNorm folded into the convs'
epilogues); nothing of the model changes.  The protocol draws a fresh ``RandomResizedCrop(224)`` +
flip per image and epoch, so features cannot be cached: the frozen forward runs ``epochs x images``
times and is the hot path.  The head is one linear layer 2048 -> classes (``torch.nn.Linear``'s
default init, fp32 master weights) whose forward and backward are ``ops.linear`` on bf16 operands
with fp32 gradient accumulation, under ``ops.cross_entropy``; SGD with momentum 0.9 (no Nesterov),
weight decay 1e-6 on weight and bias, ``lr = 0.3 x batch / 256`` on a per-step cosine to 0 (or
``multistep``).  Every evaluation scores the test set under Resize + CenterCrop by the label's
rank (``ops.eval_cross_entropy``) and reaches the host in one copy.
"""
from __future__ import annotations

import bisect
import json
import logging
import math
from typing import Callable, Dict, List, Optional, Sequence

import torch

from .. import ops

logger = logging.getLogger(__name__)

# no peer's data stream and no other evaluation runs on this seed (training/swav_eval.py KNN_SEED)
LINEAR_SEED = 2 ** 31 + 0xE7A4

DEFAULTS = dict(NUM_EPOCHS=100, BATCH_SIZE=256, TEST_EVERY_NUM_EPOCH=1, MAX_TRAIN_IMAGES=0, MAX_TEST_IMAGES=0,
                CROP_SIZE=224, RESIZE=256, CENTER_CROP=224, BASE_LR=0.3, BASE_LR_BATCH_SIZE=256, MOMENTUM=0.9,
                WEIGHT_DECAY=1e-6, SCHEDULE="cosine", VALUES=None, MILESTONES=None, SEED=LINEAR_SEED)


def learning_rate(step: int, steps_per_epoch: int, num_epochs: int, peak: float, schedule: str = "cosine",
                  values: Optional[Sequence[float]] = None, milestones: Optional[Sequence[int]] = None) -> float:
    """The learning rate of optimiser step ``step`` (0-based), updated per step.  ``cosine``:
    ``peak * (1 + cos(pi * step / total)) / 2`` over ``total = num_epochs * steps_per_epoch`` steps.
    ``multistep``: ``peak * values[i]`` with ``i`` the number of ``milestones`` (epochs) that the
    step's epoch ``step // steps_per_epoch`` has reached (``len(values) == len(milestones) + 1``)."""
    if schedule == "cosine":
        total = max(1, num_epochs * steps_per_epoch)
        return peak * 0.5 * (1.0 + math.cos(math.pi * step / total))
    if schedule == "multistep":
        if not values or milestones is None or len(values) != len(milestones) + 1:
            raise ValueError("multistep: LINEAR_EVAL.VALUES must hold one more entry than LINEAR_EVAL.MILESTONES")
        return peak * float(values[bisect.bisect_right(list(milestones), step // steps_per_epoch)])
    raise ValueError(f"LINEAR_EVAL.SCHEDULE must be 'cosine' or 'multistep', got {schedule!r}")


class LinearProbe:
    """The linear head and its optimiser.  ``weight`` [Cp, dim] / ``bias`` [Cp] are fp32 masters with
    ``Cp = num_classes`` rounded up to a multiple of 8 (the GEMM kernels' vector width); the padded
    rows start at zero, their logits are cut away before the loss, so they receive zero gradients
    and stay zero.  The gradients accumulate in fp32 straight into ``weight.grad`` / ``bias.grad``
    (``ops.linear``'s side targets)."""

    def __init__(self, num_classes: int, dim: int = 2048, device="cpu", seed: int = LINEAR_SEED,
                 momentum: float = 0.9, weight_decay: float = 1e-6):
        if num_classes < 2:
            raise ValueError(f"linear evaluation needs at least 2 classes, got {num_classes}")
        self.num_classes, self.dim = int(num_classes), int(dim)
        Cp = -(-self.num_classes // 8) * 8
        # torch.nn.Linear's default init (kaiming_uniform_(a=sqrt(5)) and the bias bound are both
        # U(-1/sqrt(fan_in), 1/sqrt(fan_in))), from a generator of our own
        g = torch.Generator().manual_seed(int(seed))
        bound = 1.0 / math.sqrt(dim)
        w = torch.zeros(Cp, dim)
        b = torch.zeros(Cp)
        w[:self.num_classes] = torch.empty(self.num_classes, dim).uniform_(-bound, bound, generator=g)
        b[:self.num_classes] = torch.empty(self.num_classes).uniform_(-bound, bound, generator=g)
        self.weight = w.to(device).requires_grad_(True)
        self.bias = b.to(device).requires_grad_(True)
        self.weight.grad = torch.zeros_like(self.weight)
        self.bias.grad = torch.zeros_like(self.bias)
        self.opt = torch.optim.SGD([self.weight, self.bias], lr=0.0, momentum=momentum, weight_decay=weight_decay,
                                   nesterov=False)

    def _logits(self, f: torch.Tensor, train: bool) -> torch.Tensor:
        x = f.detach().to(torch.bfloat16).contiguous()
        wb = self.weight.detach().to(torch.bfloat16)
        if train:  # ops.linear's backward (the side-target accumulation) runs for an input that takes a gradient
            x.requires_grad_(True)
            y = ops.linear(x, wb, self.bias.detach(), self.weight.grad, self.bias.grad)
        else:
            y = ops.OPS.gemm(x, wb, self.bias.detach(), None, False, True, 0)
        return y[:, :self.num_classes]

    def train_step(self, f: torch.Tensor, labels: torch.Tensor, lr: float) -> torch.Tensor:
        """One SGD step on one batch of features; returns the batch's mean loss (on the device)."""
        self.weight.grad.zero_()
        self.bias.grad.zero_()
        loss = ops.cross_entropy(self._logits(f, True), labels)
        loss.backward()
        for gp in self.opt.param_groups:
            gp["lr"] = lr
        self.opt.step()
        return loss.detach()

    @torch.no_grad()
    def score(self, f: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        """[loss sum, count, top-1, top-5] of one batch as a float64 device vector."""
        out = ops.eval_cross_entropy(self._logits(f, False), labels)
        return torch.stack([out["loss_sum"].double(), out["count"].double(), out["top1"].double(),
                            out["top5"].double()])


def train_linear(extract: Callable[[torch.Tensor], torch.Tensor], train_stream, test_stream, num_classes: int,
                 settings: Optional[dict] = None, device="cpu", metrics_file: Optional[str] = None,
                 extra: Optional[dict] = None, probe: Optional[LinearProbe] = None) -> List[Dict]:
    """Train the head on ``extract(images)`` over ``train_stream.epoch(e)`` for every epoch and score
    ``test_stream`` after every ``TEST_EVERY_NUM_EPOCH`` epochs and at the end.  Returns the
    evaluation records (the last one is the result); each is also appended to ``metrics_file`` as
    one JSON line with ``"eval": true``.  ``settings``: the ``LINEAR_EVAL`` keys (``DEFAULTS``)."""
    s = dict(DEFAULTS, **{k: v for k, v in (settings or {}).items() if v is not None})
    epochs, every = int(s["NUM_EPOCHS"]), max(1, int(s["TEST_EVERY_NUM_EPOCH"]))
    spe = train_stream.steps_per_epoch()
    peak = float(s["BASE_LR"]) * int(s["BATCH_SIZE"]) / int(s["BASE_LR_BATCH_SIZE"])
    if probe is None:
        probe = LinearProbe(num_classes, device=device, seed=int(s["SEED"]), momentum=float(s["MOMENTUM"]),
                            weight_decay=float(s["WEIGHT_DECAY"]))
    records, step = [], 0
    for e in range(epochs):
        loss_sum = None
        for x, y in train_stream.epoch(e):
            lr = learning_rate(step, spe, epochs, peak, str(s["SCHEDULE"]), s["VALUES"], s["MILESTONES"])
            loss = probe.train_step(extract(x), y, lr).double()
            loss_sum = loss if loss_sum is None else loss_sum + loss
            step += 1
        if (e + 1) % every and e + 1 != epochs:
            continue
        total = None
        for x, y in test_stream:
            vec = probe.score(extract(x), y)
            total = vec if total is None else total + vec
        if total is None or loss_sum is None:
            raise ValueError("linear evaluation: a stream served no image")
        # the evaluation's only device-to-host copy (the epoch's summed train loss rides along)
        ls, n, top1, top5, tl = torch.cat([total, loss_sum.reshape(1)]).cpu().tolist()
        rec = {"linear_top1": top1 / max(n, 1.0), "linear_top5": top5 / max(n, 1.0), "linear_loss": ls / max(n, 1.0),
               "linear_epoch": e + 1, "linear_train_images": len(train_stream), "linear_test_images": int(n),
               "linear_classes": int(num_classes), "linear_train_loss": tl / max(spe, 1),
               "eval": True, **(extra or {})}
        records.append(rec)
        if metrics_file:
            with open(metrics_file, "a") as f:
                f.write(json.dumps(rec) + "\n")
        logger.info(f"linear evaluation epoch {e + 1}/{epochs}: top-1 {rec['linear_top1']:.4f} top-5 "
                    f"{rec['linear_top5']:.4f} test loss {rec['linear_loss']:.4f} ({rec['linear_test_images']} images)")
    return records


def build_linear_sets(cfg) -> dict:
    """The labelled train and test sets of a config: ``DATA.TRAIN.DATA_PATHS`` and
    ``DATA.TEST.DATA_PATHS`` (``DATA_SOURCES=[disk_folder]``), labels the first-level sub-directories
    mapped by class name onto the training folder's classes (as ``swav_eval.build_knn_sets``);
    fixed-seed subsets of at most ``LINEAR_EVAL.MAX_TRAIN_IMAGES`` / ``MAX_TEST_IMAGES`` (0: all)."""
    from ..data.image_folder import ImageFolderDataset
    from .swav_eval import _paths, _subset

    le = dict(cfg.get("LINEAR_EVAL") or {})
    s = dict(DEFAULTS, **{k: v for k, v in le.items() if v is not None})
    train, test = cfg.DATA.TRAIN, cfg.DATA.get("TEST") or {}
    if not train.get("DATA_PATHS") or not test.get("DATA_PATHS"):
        raise ValueError("linear evaluation needs DATA.TRAIN.DATA_PATHS (the labelled training folder) and "
                         "DATA.TEST.DATA_PATHS (the test folder)")
    side = int(train.get("MAX_IMAGE_SIDE", 512))
    tr = ImageFolderDataset(_paths(train.DATA_PATHS), max_image_side=side)
    te = ImageFolderDataset(_paths(test.DATA_PATHS), max_image_side=side)
    tr_idx = torch.nonzero(tr.labels >= 0).reshape(-1)
    if tr_idx.numel() == 0 or len(tr.classes) < 2:
        raise ValueError(f"linear evaluation: {_paths(train.DATA_PATHS)} needs labelled files in at least two class "
                         "sub-directories")
    index = {c: i for i, c in enumerate(tr.classes)}
    remap = torch.tensor([index.get(c, -1) for c in te.classes] + [-1], dtype=torch.int64)
    te_labels = remap[te.labels]
    te_idx = torch.nonzero(te_labels >= 0).reshape(-1)
    if te_idx.numel() == 0:
        raise ValueError(f"linear evaluation: no file under {_paths(test.DATA_PATHS)} carries a training class")
    seed = int(s["SEED"])
    return {"train": tr, "test": te, "test_labels": te_labels, "num_classes": len(tr.classes),
            "train_indices": _subset(tr_idx, int(s["MAX_TRAIN_IMAGES"]), seed),
            "test_indices": _subset(te_idx, int(s["MAX_TEST_IMAGES"]), seed + 1),
            "num_workers": int(train.get("NUM_DATALOADER_WORKERS", 8)), "settings": s}


def linear_evaluate(model, sets: dict, device, metrics_file: Optional[str] = None,
                    extra: Optional[dict] = None) -> List[Dict]:
    """The linear evaluation of ``model`` over the sets of ``build_linear_sets``: a frozen-trunk
    snapshot of the model as it is, the head trained on top.  The model itself is left alone."""
    from ..data.image_folder import ImageFolderEvalStream, ImageFolderLabelledStream

    s = sets["settings"]
    B = int(s["BATCH_SIZE"])
    trunk = model.frozen_trunk()
    train = ImageFolderLabelledStream(sets["train"], B, device, indices=sets["train_indices"], size=int(s["CROP_SIZE"]),
                                      seed=int(s["SEED"]), num_workers=sets["num_workers"])
    test = ImageFolderEvalStream(sets["test"], B, device, indices=sets["test_indices"], size=int(s["CENTER_CROP"]),
                                 resize=int(s["RESIZE"]), num_workers=sets["num_workers"])
    test.labels = sets["test_labels"][sets["test_indices"]]
    try:
        return train_linear(trunk, train, test, sets["num_classes"], s, device, metrics_file, extra)
    finally:
        train.close()
        test.close()
