"""The fused MLM evaluation (``mlm_xent_eval_kernel`` in csrc/kernels/mlm_xent.hip,
``ops.mlm_eval_cross_entropy``) against a dense float64 reference: logits = t w^T + bias, per-row
loss and the label's rank with ties going to the lower index."""
import functools
import itertools

import pytest
import torch

import dedloc_amd.ops as ops
from mlm_xent_checks import E, make_case

pytestmark = pytest.mark.gpu
OPS = torch.ops.dedloc


def reference(t, w, bias, labels):
    x = t.double() @ w.double().t() + bias.double()
    live, y = labels != -100, labels.clamp(min=0)[:, None]
    xl = x.gather(1, y)
    rank = ((x > xl) | ((x == xl) & (torch.arange(x.shape[1])[None, :] < y))).sum(1)
    return x, (torch.logsumexp(x, 1) - xl[:, 0]) * live, torch.where(live, rank, torch.full_like(rank, -1))


@functools.lru_cache(maxsize=None)
def exact_case(M, V, bias_dtype):
    """Scores exact in fp32 in any accumulation order: integers in [-2, 2], three in four 0 (|score|
    < 64, where log2-unit fp32 scores resolve 2^-18), bias multiples of 0.5.  Columns 0, y - 1, y,
    y + 1, V - 1 (y = V // 2) are copies: labels 0, y, V - 1 tie with lower and higher indices."""
    g = torch.Generator().manual_seed(100 * M + V)
    draw = lambda *s: torch.randint(-2, 3, s, generator=g) * (torch.rand(s, generator=g) < 0.25)
    t, w = draw(M, E).bfloat16(), draw(V, E).bfloat16()
    bias = (torch.randint(-4, 5, (V,), generator=g) * 0.5).to(bias_dtype)
    y = V // 2
    tied = torch.tensor([0, y - 1, y + 1, V - 1])
    w[tied], bias[tied] = w[y].clone(), bias[y].clone()
    labels = torch.randint(0, V, (M,), generator=g)
    labels[0::5], labels[1::5], labels[3::5], labels[2::4] = y, 0, V - 1, -100
    if M > 1:
        labels[M - 1] = -100
    return (t, w, bias, labels) + reference(t, w, bias, labels)[1:]


# M: one lane live, a second wave, a second and a ragged last workgroup; 65536 + 257: the first M past
# the launcher's 128-row workgroups (one sub-block per wave), on the forward's 256-row ones
@pytest.mark.parametrize("M,V,bias_dtype", [
    *itertools.product([1, 65, 257, 300], [5, 64, 65, 200], [torch.bfloat16, torch.float32]),
    (65536 + 257, 65, torch.float32)])
def test_exact_ranks_and_ties(cuda, M, V, bias_dtype):
    t, w, bias, labels, rl, rr = exact_case(M, V, bias_dtype)
    args = [x.to(cuda) for x in (t, w, bias, labels)]
    loss, rank = OPS.mlm_xent_eval(*args, -100)
    assert loss.dtype == torch.float32 and rank.dtype == torch.int32
    assert torch.equal(rank.cpu().long(), rr), (rank.cpu().long() != rr).nonzero().flatten().tolist()[:8]
    err = ((loss.cpu().double() - rl).abs() / rl.abs().clamp(min=1.0)).max().item()
    print(f"mlm_xent_eval[M={M},V={V},{bias_dtype}]: max loss error {err:.3e} (bound 1e-5)")
    assert err < 1e-5 and (loss.cpu()[labels == -100] == 0).all()
    out = ops.mlm_eval_cross_entropy(*args)
    assert out["loss_sum"].dtype == torch.float64 and out["count"].dtype == torch.int64
    assert [int(out[k]) for k in ("count", "top1", "top5")] == [int((rr >= 0).sum()), int((rr == 0).sum()),
                                                                int(((rr >= 0) & (rr < 5)).sum())]


LOSS_FLOOR = 2.0 ** -17  # tests/test_mlm_xent_gpu.py's FLOOR for the forward's loss: max-abs error / max-abs reference


@functools.lru_cache(maxsize=None)
def random_case(M, V):
    """make_case's unit-scale inputs; row i's label is the column the reference ranks i % 6.
    `clear`: live rows whose label score is more than 1e-3 relative away from every other score."""
    t, w, bias, labels = make_case(M, V, "unit")
    order = (t.double() @ w.double().t() + bias.double()).topk(6, dim=1).indices
    labels = torch.where(labels == -100, labels, order[torch.arange(M), torch.arange(M) % 6])
    labels[M - 1] = -100
    x, rl, rr = reference(t, w, bias, labels)
    y = labels.clamp(min=0)[:, None]
    gap = (x - x.gather(1, y)).abs().scatter_(1, y, float("inf")).min(1).values
    return t, w, bias, labels, rl, rr, (labels != -100) & (gap > 1e-3 * x.gather(1, y)[:, 0].abs())


@pytest.mark.parametrize("M,V", [(300, 200), (257, 30000)])
def test_random_inputs_strided_rows(cuda, M, V):
    t, w, bias, labels, rl, rr, clear = random_case(M, V)
    assert clear.sum() >= 0.9 * (labels != -100).sum()  # the rank check must cover the live rows
    wide = torch.zeros(M, 2 * E, dtype=torch.bfloat16, device=cuda)
    wide[:, 64:64 + E] = t.to(cuda)
    args = (wide[:, 64:64 + E], w.to(cuda), bias.to(cuda), labels.to(cuda), -100)
    loss, rank = OPS.mlm_xent_eval(*args)
    again = OPS.mlm_xent_eval(*args)
    assert torch.equal(loss, again[0]) and torch.equal(rank, again[1])  # the same call twice: the same bits
    err = ((loss.cpu().double() - rl).abs().max() / rl.abs().max()).item()
    print(f"mlm_xent_eval random[M={M},V={V}]: loss error {err:.3e} (bound {LOSS_FLOOR:.3e}), {int(clear.sum())} rows")
    assert err <= LOSS_FLOOR
    assert torch.equal(rank.cpu().long()[clear], rr[clear])
    assert (rank.cpu()[labels == -100] == -1).all() and (rank.cpu()[labels != -100] >= 0).all()


def test_argument_errors_and_no_logits_in_memory(cuda):
    M, V = 4096, 30000
    t, w = torch.ones(M, E, dtype=torch.bfloat16, device=cuda), torch.ones(V, E, dtype=torch.bfloat16, device=cuda)
    bias, labels = torch.zeros(V, device=cuda), torch.arange(M, device=cuda)
    with pytest.raises((ValueError, RuntimeError)):
        ops.mlm_eval_cross_entropy(t[:, :64], w[:, :64], bias, labels)
    with pytest.raises(RuntimeError):
        ops.mlm_eval_cross_entropy(t, w, bias, labels[:-1])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    out = ops.mlm_eval_cross_entropy(t, w, bias, labels)
    assert int(out["count"]) == M and int(out["top1"]) == 1  # every score ties: only label 0 ranks first
    assert torch.cuda.max_memory_allocated() - before < M * V * 2  # less than the logits alone
