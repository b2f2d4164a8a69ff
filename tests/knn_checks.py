"""fp64 references for the kNN operators (dedloc::knn_topk, dedloc::knn_vote), written from their
definition: a full sort under (score descending, bank index ascending), and a plain loop over the
neighbours.  Shared by tests/test_knn_cpu.py and tests/test_knn_gpu.py."""
import math

import numpy as np
import torch


def scores64(q, bank):
    return q.double().cpu() @ bank.double().cpu().t()


def topk_reference(q, bank, k):
    """(vals fp64 [Q, k], idx int64 [Q, k]) of the bf16 inputs' exact dot products."""
    s = scores64(q, bank).numpy()
    n = s.shape[1]
    idx = np.stack([np.lexsort((np.arange(n), -row))[:k] for row in s]) if len(s) else np.zeros((0, k), np.int64)
    vals = np.take_along_axis(s, idx, 1) if len(s) else np.zeros((0, k))
    return torch.from_numpy(vals), torch.from_numpy(idx.astype(np.int64))


def exact_inputs(Q, N, D, seed, lo=-4, hi=4):
    """Integer-valued bf16 entries in [lo, hi]: with D <= 2048 every dot product is an integer below
    2^24 in magnitude (2048 * 16 = 2^15), exact in fp32 whatever the summation order."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(lo, hi + 1, (Q, D), generator=g).to(torch.bfloat16)
    bank = torch.randint(lo, hi + 1, (N, D), generator=g).to(torch.bfloat16)
    return q, bank


def order_adversary(N, D, order, seed=0):
    """q = (256, 1, 0, ...) against bank rows (a, b, 0, ...), a < 16, b < 256: score 256 a + b is
    unique and exact for N <= 4096.  ``order``: ascending / descending / random along the bank."""
    assert N <= 4096 and D >= 2
    v = torch.arange(N)
    if order == "descending":
        v = v.flip(0)
    elif order == "random":
        v = v[torch.randperm(N, generator=torch.Generator().manual_seed(seed))]
    bank = torch.zeros(N, D)
    bank[:, 0], bank[:, 1] = v // 256, v % 256
    q = torch.zeros(1, D)
    q[0, 0], q[0, 1] = 256, 1
    return q.to(torch.bfloat16), bank.to(torch.bfloat16)


def vote_reference(vals, idx, bank_labels, targets, num_classes, sigma):
    """pred, rank (lists of int) in fp64, by the definition in docs/KERNELS.md."""
    vals, idx = vals.double().cpu().tolist(), idx.cpu().tolist()
    labels, targets = bank_labels.cpu().tolist(), targets.cpu().tolist()
    preds, ranks = [], []
    for row_v, row_i, t in zip(vals, idx, targets):
        p = [0.0] * num_classes
        voted = [False] * num_classes
        for v, i in zip(row_v, row_i):
            c = labels[i]
            if 0 <= c < num_classes:
                p[c] += math.exp((v - row_v[0]) / sigma)
                voted[c] = True
        preds.append(max(range(num_classes), key=lambda c: (p[c], -c)))
        if 0 <= t < num_classes and voted[t]:
            ranks.append(sum(1 for c in range(num_classes) if p[c] > p[t] or (p[c] == p[t] and c < t)))
        else:
            ranks.append(-1)
    return preds, ranks


def hand_vote_cases():
    """Neighbour lists with equal scores (every weight exp(0) = 1, so sums are exact small integers):
    (vals [Q, 4], idx [Q, 4], bank_labels [6], targets [Q], num_classes = 3, expected pred, rank)."""
    bank_labels = torch.tensor([0, 1, 2, 1, 7, -1], dtype=torch.int32)  # 7 and -1: out of range, no vote
    idx = torch.tensor([[0, 1, 3, 2],    # classes 0 1 1 2: class 1 wins; target 1 -> rank 0
                        [0, 1, 0, 1],    # 0 1 0 1: a tie of classes 0 and 1 -> pred 0; target 1 -> rank 1
                        [0, 0, 0, 0],    # only class 0 votes; target 2 has no vote -> -1
                        [1, 2, 3, 0],    # target -1 -> -1
                        [4, 5, 2, 2],    # two neighbours out of range: class 2 alone; target 2 -> rank 0
                        [4, 5, 4, 5],    # nobody votes: pred 0, rank -1
                        [1, 3, 2, 0]],   # target 3 >= num_classes -> -1
                       dtype=torch.int32)
    vals = torch.full(idx.shape, 0.5)
    targets = torch.tensor([1, 1, 2, -1, 2, 0, 3], dtype=torch.int64)
    return vals, idx, bank_labels, targets, 3, [1, 0, 0, 1, 2, 0, 1], [0, 1, -1, -1, 0, -1, -1]
