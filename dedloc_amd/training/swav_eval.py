"""k-nearest-neighbour evaluation of a SwAV model on frozen features (the reference's
``swav/vissl/tools/nearest_neighbor_test.py`` with ``NEAREST_NEIGHBOR: {SIGMA: 0.1, TOPK: 200}``).

A labelled bank (a subset of the training images) and a labelled query set go through the model in
``eval()`` mode under the deterministic ``Resize`` + ``CenterCrop`` transform
(``data.image_folder.ImageFolderEvalStream``); the L2-normalised features meet in
``ops.knn_classify``: the fused similarity + top-k kernel (no score matrix in memory) and the
weighted vote.  The counts are summed on the device and reach the host in one copy, the shape of
``training/evaluation.py``.  Nothing of the model changes: parameters, BatchNorm running statistics
and counters, and the concurrent-pass / graph state are as before (the eval forward is one plain
trunk pass under ``no_grad``).
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch

from .. import ops

QUERY_CHUNK = 4096  # query rows per knn_classify call (bounds the kernel's candidate-list scratch)


def extract_features(model, stream, feature: str = "trunk", frozen: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """Every image of ``stream`` (an iterable of ``(images, labels)`` batches) through ``model`` in
    eval mode: L2-normalised bf16 features [n, D] (``trunk``: D = 2048, ``head``: D = 128) and their
    labels [n] int64, on the device.  The model's training flag is restored on the way out.

    ``frozen``: the trunk runs as ``model.frozen_trunk()`` (a snapshot taken here, BatchNorm folded
    into the convs' epilogues); the head's projection, where asked for, runs on its output as above."""
    if feature not in ("trunk", "head"):
        raise ValueError(f"feature must be 'trunk' or 'head', got {feature!r}")
    was_training = model.training
    feats, labels = [], []
    try:
        model.eval()
        trunk = model.frozen_trunk() if frozen else None
        with torch.no_grad():
            for x, y in stream:
                with torch.autocast(device_type=x.device.type, dtype=torch.bfloat16, enabled=x.is_cuda):
                    if trunk is None:
                        f = model.features(x, feature)
                    else:
                        f = trunk(x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last))
                        if feature == "head":
                            f = model.heads[0].projection_head(f)
                f, _ = torch.ops.dedloc.l2norm_fwd(f.to(torch.bfloat16).contiguous(), 1e-12)
                feats.append(f)
                labels.append(y)
    finally:
        model.train(was_training)
    if not feats:
        raise ValueError("extract_features: the stream served no image")
    return torch.cat(feats), torch.cat(labels)


def knn_evaluate(model, bank_stream, query_stream, k: int = 200, sigma: float = 0.1, feature: str = "trunk",
                 num_classes: int | None = None, frozen: bool = False) -> Dict[str, float]:
    """Weighted kNN accuracy of the query set against the bank.  ``num_classes`` defaults to the
    bank stream's dataset's class count.  ``knn_samples`` counts the queries that carry a class
    label; a query whose class got no vote from its neighbours is a miss.  ``frozen``: see
    ``extract_features``."""
    bank, bank_labels = extract_features(model, bank_stream, feature, frozen)
    query, targets = extract_features(model, query_stream, feature, frozen)
    if num_classes is None:
        num_classes = len(bank_stream.dataset.classes)
    k = max(1, min(int(k), bank.shape[0]))
    total = None
    for r0 in range(0, query.shape[0], QUERY_CHUNK):
        out = ops.knn_classify(query[r0:r0 + QUERY_CHUNK], bank, bank_labels, targets[r0:r0 + QUERY_CHUNK],
                               num_classes, k=k, sigma=sigma)
        vec = torch.stack([out["top1"], out["top5"], out["count"]])
        total = vec if total is None else total + vec
    top1, top5, n = total.cpu().tolist()  # the evaluation's only device-to-host copy
    return {"knn_top1": top1 / max(n, 1), "knn_top5": top5 / max(n, 1), "knn_samples": int(n),
            "knn_bank": int(bank.shape[0]), "knn_k": int(k)}


# no peer's data stream runs on this seed (training/evaluation.py EVAL_SEED, one apart)
KNN_SEED = 2 ** 31 + 0xE7A2


def _subset(candidates: torch.Tensor, limit: int, seed: int):
    """At most ``limit`` of ``candidates`` by a fixed-seed permutation, in index order."""
    if limit > 0 and candidates.numel() > limit:
        perm = torch.randperm(candidates.numel(), generator=torch.Generator().manual_seed(seed))
        candidates = candidates[perm[:limit]].sort().values
    return candidates.tolist()


def _paths(v):
    return [v] if isinstance(v, str) else list(v or [])


def build_knn_sets(cfg) -> dict:
    """The labelled bank and query sets of a config: the bank from ``NEAREST_NEIGHBOR.BANK_PATHS``
    (default ``DATA.TRAIN.DATA_PATHS``), the queries from ``DATA.TEST.DATA_PATHS`` with
    ``DATA.TEST.DATA_SOURCES=[disk_folder]``; fixed-seed subsets of at most ``MAX_BANK_IMAGES`` /
    ``MAX_TEST_IMAGES`` labelled files.  Query labels are the bank's class indices, by class name."""
    from ..data.image_folder import ImageFolderDataset

    nn_cfg = cfg.get("NEAREST_NEIGHBOR") or {}
    train, test = cfg.DATA.TRAIN, cfg.DATA.get("TEST") or {}
    sources = test.get("DATA_SOURCES") or []
    if (sources if isinstance(sources, str) else (sources or [""])[0]) != "disk_folder" or not test.get("DATA_PATHS"):
        raise ValueError("kNN evaluation needs DATA.TEST.DATA_SOURCES=[disk_folder] and DATA.TEST.DATA_PATHS="
                         "[directory, ...] for the queries")
    bank_paths = _paths(nn_cfg.get("BANK_PATHS") or train.get("DATA_PATHS"))
    if not bank_paths:
        raise ValueError("kNN evaluation needs a bank: NEAREST_NEIGHBOR.BANK_PATHS or DATA.TRAIN.DATA_PATHS")
    side = int(train.get("MAX_IMAGE_SIDE", 512))
    bank = ImageFolderDataset(bank_paths, max_image_side=side)
    query = ImageFolderDataset(_paths(test.DATA_PATHS), max_image_side=side)
    bank_idx = torch.nonzero(bank.labels >= 0).reshape(-1)
    if bank_idx.numel() == 0:
        raise ValueError(f"kNN evaluation: no labelled file (class sub-directory) under the bank {bank_paths}")
    index = {c: i for i, c in enumerate(bank.classes)}
    remap = torch.tensor([index.get(c, -1) for c in query.classes] + [-1], dtype=torch.int64)
    query_labels = remap[query.labels]  # -1 (a file directly under a root) takes the appended -1
    query_idx = torch.nonzero(query_labels >= 0).reshape(-1)
    if query_idx.numel() == 0:
        raise ValueError(f"kNN evaluation: no query under {_paths(test.DATA_PATHS)} carries one of the bank's classes")
    return {"bank": bank, "query": query, "query_labels": query_labels,
            "bank_indices": _subset(bank_idx, int(nn_cfg.get("MAX_BANK_IMAGES", 10000)), KNN_SEED),
            "query_indices": _subset(query_idx, int(nn_cfg.get("MAX_TEST_IMAGES", 5000)), KNN_SEED + 1),
            "size": int(nn_cfg.get("CENTER_CROP", 224)), "resize": int(nn_cfg.get("RESIZE", 256)),
            "batch_size": int(test.get("BATCHSIZE_PER_REPLICA", 64)),
            "num_workers": int(train.get("NUM_DATALOADER_WORKERS", 8)), "k": int(nn_cfg.get("TOPK", 200)),
            "sigma": float(nn_cfg.get("SIGMA", 0.1)), "feature": str(nn_cfg.get("FEATURE", "trunk")),
            "frozen": bool(nn_cfg.get("FROZEN_TRUNK", False))}


def knn_evaluate_sets(model, sets: dict, device) -> Dict[str, float]:
    """``knn_evaluate`` over the sets of ``build_knn_sets`` (fresh streams: every evaluation reads
    the same images in the same order)."""
    from ..data.image_folder import ImageFolderEvalStream

    kw = dict(size=sets["size"], resize=sets["resize"], num_workers=sets["num_workers"])
    bank = ImageFolderEvalStream(sets["bank"], sets["batch_size"], device, indices=sets["bank_indices"], **kw)
    query = ImageFolderEvalStream(sets["query"], sets["batch_size"], device, indices=sets["query_indices"], **kw)
    query.labels = sets["query_labels"][sets["query_indices"]]
    try:
        return knn_evaluate(model, bank, query, k=sets["k"], sigma=sets["sigma"], feature=sets["feature"],
                            frozen=sets.get("frozen", False))
    finally:
        bank.close()
        query.close()
