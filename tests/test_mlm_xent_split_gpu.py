"""The vocabulary-split forms of the fused MLM head (``splits`` of ``ops.mlm_cross_entropy`` and
``ops.mlm_eval_cross_entropy``; the split kernels of csrc/kernels/mlm_xent.hip) with forced slice
counts, against the float64 references the unsplit kernels are held to.

V = 200 is 4 vocabulary tiles with an 8-row tail: 3 slices are uneven (1, 1, 2 tiles), 5 are clamped
to 4; V = 1000 has its tail tile in the last slice; M = 257 has a ragged last 128-row block.  The
labels of make_case / exact_case fall in the first and the last slice, and rows are ignored."""
import pytest
import torch

import dedloc_amd.ops as ops
from conftest import record_margin
from mlm_xent_checks import make_case, reference, rel_errors, run_composed
from test_mlm_xent_eval_gpu import exact_case
from test_mlm_xent_gpu import FACTOR, FLOOR, NAMES

pytestmark = pytest.mark.gpu
OPS = torch.ops.dedloc


def run_split(t, w, bias, labels, splits=0):
    """forward and backward into zeroed gw / gb: (loss, dt, gw, gb)"""
    t = t.detach().clone().requires_grad_()
    gw = torch.zeros(w.shape, dtype=torch.float32, device=w.device)
    gb = torch.zeros(w.shape[0], dtype=torch.float32, device=w.device)
    loss = ops.mlm_cross_entropy(t, w, bias, labels, gw, gb, splits=splits)
    loss.backward()
    return loss.detach(), t.grad, gw, gb


@pytest.mark.parametrize("splits", [2, 3, 5])
@pytest.mark.parametrize("M,V", [(1, 200), (33, 200), (257, 1000)])
def test_training_forced_splits(cuda, M, V, splits):
    """The bound of tests/test_mlm_xent_gpu.py, unchanged: each error (max-abs error / max-abs float64
    reference) at most FACTOR x max(the composed path's error, FLOOR)."""
    case = [x.to(cuda) for x in make_case(M, V, "unit")]
    ref = reference(M, V, "unit")
    got = run_split(*case, splits=splits)
    err_f, err_c = rel_errors(got, ref), rel_errors(run_composed(ops, *case), ref)
    name = f"mlm_xent_split[M={M},V={V},splits={splits}]"
    print(name, dict(zip(NAMES, zip(err_f, err_c))))
    record_margin(name, fused=dict(zip(NAMES, err_f)), composed=dict(zip(NAMES, err_c)), factor=FACTOR)
    for what, f, c in zip(NAMES, err_f, err_c):
        assert f <= FACTOR * max(c, FLOOR), (name, what, f, c)
    for a, b in zip(got, run_split(*case, splits=splits)):  # a second identical call: identical bits
        assert torch.equal(a, b), name


@pytest.mark.parametrize("splits", [2, 3])
@pytest.mark.parametrize("bias_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("M", [65, 300])
def test_evaluation_forced_splits_exact(cuda, M, bias_dtype, splits):
    """exact_case's tied copies at columns 0, y - 1, y + 1 and V - 1 sit in other slices than label y"""
    t, w, bias, labels, rl, rr = exact_case(M, 200, bias_dtype)
    loss, rank = OPS.mlm_xent_eval(*[x.to(cuda) for x in (t, w, bias, labels)], -100, splits)
    assert torch.equal(rank.cpu().long(), rr), (rank.cpu().long() != rr).nonzero().flatten().tolist()[:8]
    err = ((loss.cpu().double() - rl).abs() / rl.abs().clamp(min=1.0)).max().item()
    print(f"mlm_xent_eval[M={M},V=200,{bias_dtype},splits={splits}]: max loss error {err:.3e} (bound 1e-5)")
    assert err < 1e-5 and (loss.cpu()[labels == -100] == 0).all()


def test_one_split_is_the_default_and_negative_raises(cuda):
    M, V = 65, 200  # 4 vocabulary tiles: the automatic rule does not split
    case = [x.to(cuda) for x in make_case(M, V, "unit")]
    for a, b in zip(run_split(*case), run_split(*case, splits=1)):
        assert torch.equal(a, b)
    for a, b in zip(OPS.mlm_xent_eval(*case, -100), OPS.mlm_xent_eval(*case, -100, 1)):
        assert torch.equal(a, b)
    with pytest.raises((ValueError, RuntimeError)):
        ops.mlm_cross_entropy(*case, splits=-1)
    with pytest.raises((ValueError, RuntimeError)):
        ops.mlm_eval_cross_entropy(*case, splits=-1)
    with pytest.raises(RuntimeError):
        OPS.mlm_xent_eval(*case, -100, -1)
