"""The ``xent_eval`` HIP kernel (csrc/kernels/xent_eval.hip) against the plain-torch oracle of
tests/test_xent_eval_cpu.py on the same bf16 logits: ranks exactly, per-row loss within
``1e-3 * max(1, |ref|)`` (the bound tests/test_kernels_gpu.py::test_xent holds this arithmetic to)."""
import functools
import importlib.util
import math
import os

import pytest
import torch

import dedloc_amd.ops as ops
from conftest import record_margin

pytestmark = pytest.mark.gpu
OPS = torch.ops.dedloc

_spec = importlib.util.spec_from_file_location(
    "_xent_eval_oracle", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_xent_eval_cpu.py"))
_cpu = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_cpu)
oracle, make_case, tie_rows = _cpu.oracle, _cpu.make_case, _cpu.tie_rows

M = 67
# 2: SOP, 254 of 256 threads own nothing; 509: prime, rows start off the 16-byte grid (scalar edges);
# 512: the tiny vocabulary; 2048: exactly one 8-wide load per thread; 2056: one ragged extra stride;
# 30000: 3750 vectors, ragged last stride; 31995: odd (the sahajBERT vocabulary), scalar edges
VS = [2, 509, 512, 2048, 2056, 30000, 31995]
LOSS_RTOL = 1e-3


@functools.lru_cache(maxsize=None)
def _case(V):
    """(logits, labels, oracle loss, oracle rank) on the host, computed once per V and never changed."""
    x, lab = make_case(M, V, seed=V)
    return (x, lab) + oracle(x, lab)


def _check(name, x, lab, loss, rank, rl, rr):
    loss, rank = loss.cpu(), rank.cpu()
    assert rank.dtype == torch.int32 and loss.dtype == torch.float32
    assert torch.equal(rank, rr), (name, (rank != rr).nonzero().flatten().tolist()[:8])
    ign = lab.cpu() == -100
    assert (loss[ign] == 0).all() and (rank[ign] == -1).all()
    err = ((loss - rl).abs() / rl.abs().clamp(min=1.0)).max().item() if loss.numel() else 0.0
    print(f"{name}: max loss error {err:.3e} (bound {LOSS_RTOL})")
    record_margin(name, max_rel_loss_err=err, bound=LOSS_RTOL)
    assert err < LOSS_RTOL, (name, err)


@pytest.mark.parametrize("V", VS)
def test_xent_eval_matches_oracle(cuda, V):
    x, lab, rl, rr = _case(V)
    loss, rank = OPS.xent_eval(x.to(cuda), lab.to(cuda), -100)
    _check(f"xent_eval[V={V}]", x, lab, loss, rank, rl, rr)


@pytest.mark.parametrize("V", VS)
def test_xent_eval_first_last_ignored_and_end_labels(cuda, V):
    x = _case(V)[0]
    lab = _case(V)[1].clone()
    lab[0], lab[-1] = -100, -100
    lab[1:-1:2], lab[2:-1:2] = 0, V - 1
    rl, rr = oracle(x, lab)
    loss, rank = OPS.xent_eval(x.to(cuda), lab.to(cuda), -100)
    _check(f"xent_eval_ends[V={V}]", x, lab, loss, rank, rl, rr)


@pytest.mark.parametrize("V", VS)
def test_xent_eval_ties(cuda, V):
    x, lab = tie_rows(V)
    rl, rr = oracle(x, lab)
    loss, rank = OPS.xent_eval(x.to(cuda), lab.to(cuda), -100)
    _check(f"xent_eval_ties[V={V}]", x, lab, loss, rank, rl, rr)
    assert int(rank[0]) == int(lab[0])  # all-equal logits: the rank is the label's index
    assert abs(float(loss[0]) - math.log(V)) < LOSS_RTOL * max(1.0, math.log(V))
    assert int(rank[1]) == 1  # one equal maximum before the label, one after
    assert math.isfinite(float(loss[2]))  # -inf off the label


def test_xent_eval_empty_single_all_ignored(cuda):
    x, lab, rl, rr = _case(512)
    xg, lg = x.to(cuda), lab.to(cuda)
    l0, r0 = OPS.xent_eval(xg[:0], lg[:0], -100)
    assert l0.shape == (0,) and r0.shape == (0,)
    out0 = ops.eval_cross_entropy(xg[:0], lg[:0])
    assert float(out0["loss_sum"]) == 0.0 and int(out0["count"]) == 0 and int(out0["top1"]) == 0
    l1, r1 = OPS.xent_eval(xg[1:2], lg[1:2], -100)
    _check("xent_eval[M=1]", x[1:2], lab[1:2], l1, r1, rl[1:2], rr[1:2])
    la, ra = OPS.xent_eval(xg, torch.full_like(lg, -100), -100)
    assert (la == 0).all() and (ra == -1).all()
    outa = ops.eval_cross_entropy(xg, torch.full_like(lg, -100))
    assert float(outa["loss_sum"]) == 0.0 and int(outa["count"]) == 0 and int(outa["top5"]) == 0


@pytest.mark.parametrize("V", [512, 30000, 31995])
def test_eval_cross_entropy_reproducible_and_agrees_with_training_kernel(cuda, V):
    x, lab, rl, rr = _case(V)
    xg, lg = x.to(cuda), lab.to(cuda)
    a, b = ops.eval_cross_entropy(xg, lg), ops.eval_cross_entropy(xg, lg)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert int(a["count"]) == int((lab != -100).sum())
    assert int(a["top1"]) == int((rr == 0).sum()) and int(a["top5"]) == int(((rr >= 0) & (rr < 5)).sum())
    mean = float(a["loss_sum"]) / int(a["count"])
    train = float(OPS.xent_fwd_bwd(xg, lg, False, -100)[0])
    err = abs(mean - train) / max(1.0, abs(train))
    print(f"eval mean {mean:.6f} training kernel {train:.6f}: error {err:.3e} (bound {LOSS_RTOL})")
    record_margin(f"xent_eval_vs_fwd_bwd[V={V}]", rel_err=err, bound=LOSS_RTOL)
    assert err < LOSS_RTOL


@pytest.mark.parametrize("V,ld,front", [(512, 512, 1024), (512, 512, 1001), (509, 509, 1000), (2, 2, 999),
                                        (2048, 2056, 4096), (509, 517, 1001)])
def test_xent_eval_stays_inside_its_rows(cuda, V, ld, front):
    """The logits sit inside a larger buffer filled with a guard value (rows ``ld`` apart, guard
    columns between them when ld > V): results match the oracle — so nothing outside the rows was
    read into them, not for ignored rows' labels either — and the buffer is bit-unchanged."""
    x, lab, rl, rr = _case(V)
    guard = 30000.0  # any guard element read as a logit would dominate the row's logsumexp and rank
    buf = torch.full((front + M * ld + 4096,), guard, dtype=torch.bfloat16, device=cuda)
    view = buf[front:front + M * ld].view(M, ld)[:, :V]
    view.copy_(x.to(cuda))
    before = buf.clone()
    loss, rank = OPS.xent_eval(view, lab.to(cuda), -100)
    _check(f"xent_eval_guard[V={V},ld={ld}]", x, lab, loss, rank, rl, rr)
    assert torch.equal(buf.view(torch.int16), before.view(torch.int16))
