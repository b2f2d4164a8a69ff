"""Inputs and the float64 reference shared by tests/test_mlm_xent_cpu.py and test_mlm_xent_gpu.py.

Reference: the same bf16 inputs taken to float64 on the CPU, logits = t @ w.T + bias,
``F.cross_entropy(ignore_index=-100)`` and autograd for dt, dw, dbias."""
import functools

import torch
import torch.nn.functional as F

E = 128


@functools.lru_cache(maxsize=None)
def make_case(M, V, family, all_ignored=False):
    """(t, w, bias, labels) on the host.  Labels: row 0 is labelled 0, row M - 1 is labelled V - 1
    (the tail tile), about a quarter of the rows are -100.  family "unit": unit-scale logits, bf16
    bias; "big": logits reach about +-60, row 0 peaks at vocabulary row V - 1 (its running maximum
    grows in the last tile) and row M - 1 at row 0, each away from its own label so that the
    gradient stays of order 1 / rows; fp32 bias of bf16-representable values."""
    g = torch.Generator().manual_seed(1000 * M + V)
    w = torch.randn(V, E, generator=g) / E ** 0.5
    t = torch.randn(M, E, generator=g)
    bias = (0.5 * torch.randn(V, generator=g)).bfloat16()
    if family == "big":
        t = t * 20.0
        t[0] = w[V - 1] * (60.0 / w[V - 1].pow(2).sum())
        t[M - 1] = w[0] * (60.0 / w[0].pow(2).sum())
        bias = bias.float()
    labels = torch.randint(0, V, (M,), generator=g)
    labels[torch.arange(M) % 4 == 2] = -100
    labels[0] = 0
    labels[M - 1] = V - 1
    if all_ignored:
        labels[:] = -100
    return t.bfloat16(), w.bfloat16(), bias, labels


@functools.lru_cache(maxsize=None)
def reference(M, V, family, all_ignored=False):
    """float64 (loss, dt, dw, dbias) of make_case's inputs; computed once, never changed."""
    t, w, bias, labels = make_case(M, V, family, all_ignored)
    t, w, bias = (x.double().requires_grad_() for x in (t, w, bias))
    if all_ignored:  # F.cross_entropy gives nan (0 / 0); the ops give 0 and zero gradients
        return torch.zeros((), dtype=torch.float64), torch.zeros_like(t), torch.zeros_like(w), torch.zeros_like(bias)
    loss = F.cross_entropy(t @ w.t() + bias, labels, ignore_index=-100)
    return (loss.detach(),) + torch.autograd.grad(loss, (t, w, bias))


def rel_errors(got, ref):
    """max-abs error / max-abs reference, for each of (loss, dt, dw, dbias)"""
    return [((g.detach().double().cpu() - r).abs().max() / r.abs().max().clamp(min=1e-30)).item()
            for g, r in zip(got, ref)]


def run_fused(ops, t, w, bias, labels, fill=0.25):
    """ops.mlm_cross_entropy forward and backward into gw / gb pre-filled with `fill`:
    (loss, dt, gw - fill, gb - fill), and the raw tensors for bit comparisons"""
    t = t.detach().clone().requires_grad_()
    gw = torch.full(w.shape, fill, dtype=torch.float32, device=w.device)
    gb = torch.full((w.shape[0],), fill, dtype=torch.float32, device=w.device)
    loss = ops.mlm_cross_entropy(t, w, bias, labels, gw, gb)
    loss.backward()
    return (loss, t.grad, gw - fill, gb - fill), (loss.detach(), t.grad, gw, gb)


def run_composed(ops, t, w, bias, labels):
    """ops.linear then ops.cross_entropy on the same inputs: (loss, dt, dw, dbias)"""
    t = t.detach().clone().requires_grad_()
    gw = torch.zeros(w.shape, dtype=torch.float32, device=w.device)
    gb = torch.zeros(w.shape[0], dtype=torch.float32, device=w.device)
    loss = ops.cross_entropy(ops.linear(t, w, bias, gw, gb), labels)
    loss.backward()
    return loss, t.grad, gw, gb
