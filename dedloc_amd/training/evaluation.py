"""Local evaluation on held-out data (the reference hands ``tokenized_datasets["validation"]`` to
its HF ``Trainer`` under ``--do_eval``, albert/run_trainer.py:278).

The held-out stream is rebuilt from one fixed seed at the start of every evaluation, so every
evaluation on every peer (and on the coordinator's replica) scores the same instances under the
same mask: the numbers are comparable between peers and between steps, which the training loss —
masked anew every batch, per-peer data — is not.  Statistics are summed on the device by
``AlbertForPreTraining.evaluate_batch`` (the forward-only ``xent_eval`` kernel: loss and the
label's rank from one read of the logits) and copied to the host once per evaluation.
"""
from __future__ import annotations

import math
from typing import Callable, Dict

import torch

from ..data.sop_dataset import DiskSOPStream
from ..data.synthetic_mlm import SyntheticSOPStream

# peer_seed() is a residue modulo 2**31, so no peer's training stream can run on this seed
EVAL_SEED = 2 ** 31 + 0xE7A1

_KEYS = ("mlm_loss_sum", "mlm_count", "mlm_top1", "mlm_top5", "sop_loss_sum", "sop_count", "sop_correct")


def build_eval_stream(dataset_args, training_args, vocab_size: int, device):
    """The held-out stream at ``per_device_eval_batch_size``: ``--eval_dataset_path`` (a directory
    built by data/sop_dataset.py from held-out documents) or, without one, a synthetic stream with
    the run's ``mask_mode`` / ``length_mode`` / ``pattern_period``.  Always seeded with EVAL_SEED."""
    B = int(training_args.per_device_eval_batch_size)
    path = getattr(dataset_args, "eval_dataset_path", None)
    if path:
        return DiskSOPStream(path, B, seed=EVAL_SEED, device=device)
    return SyntheticSOPStream(B, training_args.seq_length, vocab_size, seed=EVAL_SEED, device=device,
                              mask_mode=getattr(dataset_args, "mask_mode", "fixed"),
                              length_mode=getattr(dataset_args, "length_mode", "full"),
                              pattern_period=getattr(dataset_args, "pattern_period", 0))


def evaluate(model, make_stream: Callable[[], object], num_batches: int) -> Dict[str, float]:
    """``num_batches`` batches of a fresh ``make_stream()`` through ``model.evaluate_batch``; the sums
    stay on the device and reach the host in one copy at the end.  ``eval_loss`` is the sum of the
    two component means, as in ``forward``."""
    stream = make_stream()
    packed = bool(getattr(model, "pack_sequences", False))
    total = None
    for _ in range(int(num_batches)):
        batch = stream.next_batch()
        out = model.evaluate_batch(batch, lengths=getattr(stream, "last_lengths", None) if packed else None)
        vec = torch.stack([out[k].to(torch.float64) for k in _KEYS])
        total = vec if total is None else total + vec
    if total is None:
        raise ValueError("evaluate() needs num_batches >= 1")
    t = dict(zip(_KEYS, total.cpu().tolist()))  # the evaluation's only device-to-host copy
    mlm_n, sop_n = max(t["mlm_count"], 1.0), max(t["sop_count"], 1.0)
    mlm_loss, sop_loss = t["mlm_loss_sum"] / mlm_n, t["sop_loss_sum"] / sop_n
    return {"eval_loss": mlm_loss + sop_loss, "eval_mlm_loss": mlm_loss, "eval_sop_loss": sop_loss,
            "eval_mlm_accuracy": t["mlm_top1"] / mlm_n, "eval_mlm_top5": t["mlm_top5"] / mlm_n,
            "eval_sop_accuracy": t["sop_correct"] / sop_n,
            "eval_perplexity": math.exp(min(mlm_loss, 700.0)), "eval_samples": int(t["sop_count"])}
