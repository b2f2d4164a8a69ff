"""The ``dedloc::xent_eval`` CPU reference op and ``ops.eval_cross_entropy`` against a plain-torch
oracle written here: ``torch.logsumexp`` in fp32, and the label's rank by its comparison formula
(row by row, so it shares no vectorised expression with the implementation)."""
import math

import pytest
import torch

import dedloc_amd.ops as ops

OPS = torch.ops.dedloc


def oracle(logits, labels, ignore_index=-100):
    """(loss fp32 [M], rank int32 [M]) of bf16 ``logits`` [M, V]: loss = logsumexp(x) - x[label], rank =
    #{j : x[j] > x[label] or (x[j] == x[label] and j < label)}; ignored rows are (0, -1)."""
    x = logits.detach().float().cpu()
    lab = labels.detach().cpu().tolist()
    loss = torch.zeros(len(lab), dtype=torch.float32)
    rank = torch.full((len(lab),), -1, dtype=torch.int32)
    for r, y in enumerate(lab):
        if y == ignore_index:
            continue
        row = x[r]
        loss[r] = torch.logsumexp(row, 0) - row[y]
        rank[r] = int((row > row[y]).sum()) + int((row[:y] == row[y]).sum())
    return loss, rank


def make_case(M, V, seed=0, ignore_every=7):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, V, generator=g) * 3).bfloat16()
    lab = torch.randint(0, V, (M,), generator=g)
    if ignore_every:
        lab[::ignore_every] = -100
    return x, lab


def tie_rows(V):
    """Rows built to tie: all-equal logits; the row maximum both before and after the label's equal
    value; -inf everywhere but the label and one other column."""
    a = max(1, V // 3)
    equal = torch.full((V,), 1.5)
    around = torch.randn(V, generator=torch.Generator().manual_seed(5)).clamp(max=2.0)
    around[[0, a, V - 1]] = 4.0  # three equal maxima: one before, the label, one after
    ninf = torch.full((V,), -math.inf)
    ninf[a] = 0.25
    ninf[V - 1] = 1.0
    x = torch.stack([equal, around, ninf]).bfloat16()
    return x, torch.tensor([a, a, a])


@pytest.mark.parametrize("V", [2, 509, 512, 2056])
def test_xent_eval_cpu_matches_oracle(V):
    x, lab = make_case(67, V)
    loss, rank = OPS.xent_eval(x, lab, -100)
    rl, rr = oracle(x, lab)
    assert loss.dtype == torch.float32 and rank.dtype == torch.int32
    assert torch.equal(rank, rr)
    assert torch.allclose(loss, rl, rtol=1e-6, atol=1e-6)
    assert (loss[::7] == 0).all() and (rank[::7] == -1).all()


def test_xent_eval_cpu_edges():
    V = 512
    x, lab = make_case(9, V, ignore_every=0)
    lab[0], lab[-1], lab[1], lab[2] = -100, -100, 0, V - 1
    loss, rank = OPS.xent_eval(x, lab, -100)
    rl, rr = oracle(x, lab)
    assert torch.equal(rank, rr) and torch.allclose(loss, rl, rtol=1e-6, atol=1e-6)
    # ties: lower index wins
    xt, lt = tie_rows(V)
    loss, rank = OPS.xent_eval(xt, lt, -100)
    rl, rr = oracle(xt, lt)
    assert torch.equal(rank, rr) and torch.allclose(loss, rl, rtol=1e-6, atol=1e-6)
    assert rank[0] == lt[0] and loss[0] == pytest.approx(math.log(V), rel=1e-6)
    assert rank[1] == 1 and rank[2] == 1
    # empty, one row, everything ignored
    l0, r0 = OPS.xent_eval(x[:0], lab[:0], -100)
    assert l0.shape == (0,) and r0.shape == (0,)
    l1, r1 = OPS.xent_eval(x[1:2], lab[1:2], -100)
    assert torch.equal(r1, rr.new_tensor([int(oracle(x[1:2], lab[1:2])[1])]))
    la, ra = OPS.xent_eval(x, torch.full((9,), -100), -100)
    assert (la == 0).all() and (ra == -1).all()


def test_eval_cross_entropy_cpu():
    x, lab = make_case(67, 512)
    rl, rr = oracle(x, lab)
    out = ops.eval_cross_entropy(x, lab)
    again = ops.eval_cross_entropy(x, lab)
    assert set(out) == {"loss_sum", "count", "top1", "top5"}
    assert all(torch.equal(out[k], again[k]) for k in out)
    assert int(out["count"]) == int((lab != -100).sum())
    assert int(out["top1"]) == int((rr == 0).sum())
    assert int(out["top5"]) == int(((rr >= 0) & (rr < 5)).sum())
    assert float(out["loss_sum"]) == pytest.approx(float(rl.double().sum()), rel=1e-6)
    # the mean agrees with the training op's loss on the same input
    mean = float(out["loss_sum"]) / int(out["count"])
    assert mean == pytest.approx(float(OPS.xent_fwd_bwd(x, lab, False, -100)[0]), rel=1e-5)
    # other k, and a strided 2-D view of wider rows
    wide = torch.full((67, 520), 9.0).bfloat16()
    wide[:, :512] = x
    out3 = ops.eval_cross_entropy(wide[:, :512], lab, topk=(3,))
    assert set(out3) == {"loss_sum", "count", "top3"} and int(out3["top3"]) == int(((rr >= 0) & (rr < 3)).sum())
    assert torch.equal(out3["loss_sum"], out["loss_sum"])
