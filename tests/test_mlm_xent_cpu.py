"""CPU tier of the fused MLM head: the CPU implementations of ``dedloc::mlm_xent_fwd`` / ``_bwd``
(fp32 torch, dS rounded to bf16 as the kernels pack it) against the float64 reference of
tests/mlm_xent_checks.py, and the model switch ``_FUSED_MLM_LOSS``.

Bounds (max-abs error / max-abs reference), from the number formats: loss and dbias are fp32 sums
of fp32 terms (1e-5); dw sums bf16-rounded dS (2^-9 each) in fp32 (2^-8); dt does too and is stored
as bf16 (2^-7)."""
import pytest
import torch

import dedloc_amd.ops as ops
from mlm_xent_checks import make_case, reference, rel_errors, run_fused

BOUNDS = (1e-5, 2.0 ** -7, 2.0 ** -8, 1e-5)


@pytest.mark.parametrize("M,V,family", [(33, 112, "unit"), (65, 200, "big")])
def test_cpu_ops_match_float64(M, V, family):
    fused, _ = run_fused(ops, *make_case(M, V, family))
    errs = rel_errors(fused, reference(M, V, family))
    print(errs)
    for e, b in zip(errs, BOUNDS):
        assert e <= b, (errs, BOUNDS)


def test_cpu_every_row_ignored():
    fused, _ = run_fused(ops, *make_case(33, 112, "unit", True))
    assert rel_errors(fused, reference(33, 112, "unit", True)) == [0.0] * 4


def test_rejects_other_embedding_sizes():
    with pytest.raises(ValueError):
        ops.mlm_cross_entropy(torch.zeros(4, 64).bfloat16(), torch.zeros(8, 64).bfloat16(), torch.zeros(8),
                              torch.zeros(4, dtype=torch.long))


def test_model_switch_cpu(monkeypatch):
    """Fused and composed arms on the same batch: bounds as tests/test_mlm_xent_gpu.py derives them."""
    from dedloc_amd.models import albert

    cfg = albert.AlbertConfig.tiny(vocab_size=500, embedding_size=128, num_hidden_layers=2,
                                   classifier_dropout_prob=0.0)
    torch.manual_seed(0)
    model = albert.AlbertForPreTraining(cfg)
    model.materialize(torch.device("cpu"))
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(5, cfg.vocab_size, (2, 64), generator=g)
    labels = torch.where(torch.rand(2, 64, generator=g) < 0.2, ids, torch.full((2, 64), -100))
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(albert, "_FUSED_MLM_LOSS", fused)
        model.flat.zero_grad()
        out = model(ids, labels=labels, sentence_order_label=torch.tensor([0, 1]))
        out["loss"].backward()
        res[fused] = (out["mlm_loss"].item(), model.flat.grad.clone())
    (la, ga), (lb, gb) = res[True], res[False]
    assert abs(la - lb) <= 2.0 ** -8 * abs(lb), (la, lb)
    assert ((ga - gb).norm() / gb.norm()).item() <= 2.0 ** -7
    out = model(ids, labels=labels, return_logits=True)
    assert out["prediction_logits_masked"].shape == (int((labels != -100).sum()), cfg.vocab_size)
