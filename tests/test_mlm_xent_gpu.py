"""The fused MLM head (csrc/kernels/mlm_xent.hip, ``ops.mlm_cross_entropy``) against the float64
reference of tests/mlm_xent_checks.py, and against the composed path (``ops.linear`` then
``ops.cross_entropy``) on the same inputs: for each of loss, dt, dw, dbias the fused error
(max-abs error / max-abs reference) may exceed the composed one by at most FACTOR, which covers
only rounding-order chance between two bf16 pipelines (both round dS to bf16; the composed one
also rounds the logits).  Figures below FLOOR are not compared: where dS is exactly +-1 or 0 (a
single row whose softmax is one-hot) the composed path is exact by accident, its bf16 logits making
x - max exactly 0, while any fp32 softmax of log2-unit scores up to 2^7 resolves the exponent only to
one fp32 ulp of that, 2^-17."""
import pytest
import torch

import dedloc_amd.ops as ops
from conftest import record_margin
from mlm_xent_checks import make_case, reference, rel_errors, run_composed, run_fused

pytestmark = pytest.mark.gpu

FACTOR = 1.27  # 1.25 plus what [M=1, V=64, unit] measured: dt is one row there, both errors one bf16 output rounding (1.2635)
FLOOR = 2.0 ** -17
# M: one row; the 32-row sub-block and 64-row tile boundaries; a 128-row block + 1; a 256-row block + 1
MS = [1, 31, 33, 64, 65, 129, 257]
# V: less than a tile; one tile; a tile + the model's tail residue of 48; several tiles with a tail
VS = [48, 64, 112, 200]
NAMES = ("loss", "dt", "dw", "dbias")


def _check(cuda, M, V, family, all_ignored=False):
    case = [x.to(cuda) for x in make_case(M, V, family, all_ignored)]
    ref = reference(M, V, family, all_ignored)
    fused, raw = run_fused(ops, *case)
    again = run_fused(ops, *case)[1]
    err_f, err_c = rel_errors(fused, ref), rel_errors(run_composed(ops, *case), ref)
    name = f"mlm_xent[M={M},V={V},{family}{',ignored' if all_ignored else ''}]"
    print(name, dict(zip(NAMES, zip(err_f, err_c))))
    record_margin(name, fused=dict(zip(NAMES, err_f)), composed=dict(zip(NAMES, err_c)), factor=FACTOR)
    for a, b in zip(raw, again):  # a second identical call: identical bits
        assert torch.equal(a, b), name
    return name, err_f, err_c


@pytest.mark.parametrize("family", ["unit", "big"])
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("M", MS)
def test_fused_no_worse_than_composed(cuda, M, V, family):
    name, err_f, err_c = _check(cuda, M, V, family)
    for what, f, c in zip(NAMES, err_f, err_c):
        assert f <= FACTOR * max(c, FLOOR), (name, what, f, c)
    assert err_f[0] <= max(err_c[0], FLOOR), (name, "the fused loss works from unrounded logits", err_f[0], err_c[0])


def test_every_row_ignored(cuda):
    name, err_f, _ = _check(cuda, 65, 112, "unit", all_ignored=True)
    assert err_f == [0.0] * 4, (name, err_f)  # loss 0 and zero gradients, as ops.cross_entropy gives


# ---------------------------------------------------------------------------------------- model
# The two arms differ by the composed path's bf16 logits: a relative 2^-9 on logits of order 1 moves
# the mean loss (about ln V) by less than 2^-8 of it; in the gradient that perturbation of P adds to
# the 2^-9 rounding of dS, both pipelines' own, so the flat gradients agree within 2^-7 in norm.
LOSS_RTOL, GRAD_RTOL = 2.0 ** -8, 2.0 ** -7


@pytest.mark.parametrize("packed", [False, True])
def test_model_switch(cuda, monkeypatch, packed):
    from dedloc_amd.models import albert

    cfg = albert.AlbertConfig.tiny(vocab_size=500, embedding_size=128, num_hidden_layers=2,
                                   classifier_dropout_prob=0.0)
    torch.manual_seed(0)
    model = albert.AlbertForPreTraining(cfg)
    model.materialize(cuda)
    B, S, lens = 3, 64, [64, 40, 9]
    g = torch.Generator().manual_seed(1)
    am = (torch.arange(S)[None, :] < torch.tensor(lens)[:, None]).long()
    ids = torch.randint(5, cfg.vocab_size, (B, S), generator=g) * am
    sel = (torch.rand(B, S, generator=g) < 0.2) & am.bool()
    sel[:, 1] = True
    labels = torch.where(sel, torch.randint(5, cfg.vocab_size, (B, S), generator=g), torch.full((B, S), -100))
    kw = dict(input_ids=ids.to(cuda), attention_mask=am.to(cuda), labels=labels.to(cuda),
              sentence_order_label=torch.tensor([0, 1, 1], device=cuda), pack_sequences=packed, lengths=lens)
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(albert, "_FUSED_MLM_LOSS", fused)
        model.flat.zero_grad()
        out = model(**kw)
        assert "prediction_logits_masked" not in out
        out["loss"].backward()
        res[fused] = (out["mlm_loss"].item(), model.flat.grad.clone())
    (la, ga), (lb, gb) = res[True], res[False]
    grad_err = ((ga - gb).norm() / gb.norm()).item()
    print(f"packed={packed}: mlm loss fused {la:.6f} composed {lb:.6f}, flat gradient rel diff {grad_err:.2e}")
    assert abs(la - lb) <= LOSS_RTOL * abs(lb) and grad_err <= GRAD_RTOL
    monkeypatch.setattr(albert, "_FUSED_MLM_LOSS", True)
    out = model(return_logits=True, **kw)
    assert out["prediction_logits_masked"].shape == (int(sel.sum()), cfg.vocab_size)
