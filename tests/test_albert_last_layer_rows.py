"""AlbertForPreTraining with its last layer on the rows the heads read (``_LAST_LAYER_ROWS``,
models/albert.py: _AlbertLastLayerFn over ops.attn_fwd_q / attn_bwd_q) against the full last layer.

Tiny config (hidden 128, 2 heads of 64, 3 applications of the shared layer), B = 3, S = 128, one
right-padded sequence and one sequence without any MLM target; on the CPU reference ops and on the
GPU kernels.  With the switch on and off:
  * the forward is equal: the MLM logits of every target row and the SOP logits bit for bit, and
    the losses equal.  On the GPU the loss scalars are held to 64 * 2^-24 relative instead: the
    cross-entropy kernels add the rows' losses with fp32 atomics in arrival order, so the full
    layer's own loss differs between two runs on one input in the last place (measured on an
    MI355X: 6.969865322 and 6.969864845), and reordering a sum of n <= 60 positive terms moves it by
    at most n * 2^-24 of its value.  The logits carry the claim row by row;
  * every parameter gradient is within the norm-wise bound tests/test_albert_model.py holds its two
    paths to (3e-2 of the tensor's gradient norm, floored at 1e-5 of the total norm), here for every
    tensor whatever its size; the two runs differ by the order of the fp32 sums only (measured on
    the CPU ops: 3e-6 of the flat gradient);
  * ``evaluate_batch`` returns the same statistics;
for both MLM target forms.  ``encode()`` called directly still returns every row, and a packed
batch and a head_dim-128 config run the full layer."""
import math

import pytest
import torch

import dedloc_amd.models.albert as albert
from dedloc_amd.models.albert import AlbertConfig, AlbertForPreTraining

B, S, P = 3, 128, 20
DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]


@pytest.fixture
def device(request):
    if request.param == "cuda":
        return request.getfixturevalue("cuda")
    return torch.device("cpu")


def _batch(V, device, form):
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(5, V, (B, S), generator=g)
    ids[:, 0] = 2
    am = torch.ones(B, S, dtype=torch.long)
    am[1, 90:] = 0
    ids[1, 90:] = 0
    tt = torch.zeros(B, S, dtype=torch.long)
    tt[:, S // 3:] = 1
    tt *= am
    batch = {"input_ids": ids, "attention_mask": am, "token_type_ids": tt,
             "sentence_order_label": torch.randint(0, 2, (B,), generator=g)}
    if form == "labels":
        sel = (torch.rand(B, S, generator=g) < 0.15) & am.bool()
        sel[:, 0] = False
        sel[2] = False  # a sequence without MLM targets
        labels = torch.full((B, S), -100, dtype=torch.long)
        labels[sel] = torch.randint(5, V, (int(sel.sum()),), generator=g)
        batch["labels"] = labels
    else:
        pos = torch.stack([torch.randperm(80, generator=g)[:P] + 1 for _ in range(B)])
        lab = torch.randint(5, V, (B, P), generator=g)
        lab[0, P - 5:] = -100  # unused entries: position 0, label -100 (the streams' convention)
        pos[0, P - 5:] = 0
        lab[2] = -100  # a sequence without MLM targets
        pos[2] = 0
        batch["mlm_positions"], batch["mlm_labels"] = pos, lab
    return {k: v.to(device) for k, v in batch.items()}


def _model(device, **cfg):
    torch.manual_seed(0)
    m = AlbertForPreTraining(AlbertConfig.tiny(**cfg))
    m.materialize(device)
    m.eval()  # no classifier dropout: both runs see the same function
    return m


def _step(m, b, **kw):
    m.flat.zero_grad()
    out = m(b["input_ids"], b["attention_mask"], b["token_type_ids"], labels=b.get("labels"),
            sentence_order_label=b["sentence_order_label"], mlm_positions=b.get("mlm_positions"),
            mlm_labels=b.get("mlm_labels"), return_logits=True, **kw)
    out["loss"].backward()
    return out, {n: m.flat.g(n).detach().float().clone() for n in m.flat.names}


@pytest.fixture
def count_compact(monkeypatch):
    """How many times the compact-query attention ran."""
    calls = []
    real = albert.ops.attn_fwd_q

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(albert.ops, "attn_fwd_q", spy)
    return calls


@pytest.mark.parametrize("device", DEVICES, indirect=True)
@pytest.mark.parametrize("form", ["labels", "positions"])
def test_loss_and_gradients_match_full_last_layer(device, form, monkeypatch, count_compact):
    m = _model(device)
    b = _batch(m.config.vocab_size, device, form)
    monkeypatch.setattr(albert, "_LAST_LAYER_ROWS", False)
    out0, g0 = _step(m, b)
    ev0 = m.evaluate_batch(b)
    assert not count_compact
    monkeypatch.setattr(albert, "_LAST_LAYER_ROWS", True)
    out1, g1 = _step(m, b)
    ev1 = m.evaluate_batch(b)
    assert len(count_compact) == 2  # forward and evaluate_batch
    # reordering the kernels' atomic sum of the rows' losses (GPU only): n * 2^-24 relative, n <= 60
    slack = 64 * 2.0 ** -24 if device.type == "cuda" else 0.0
    assert out0["prediction_logits_masked"].shape[0] <= 60
    for k in ("loss", "mlm_loss", "sop_loss"):
        a, c = float(out0[k].detach()), float(out1[k].detach())
        print(k, a, c)
        assert abs(a - c) <= slack * abs(a), k
    assert torch.equal(out0["prediction_logits_masked"], out1["prediction_logits_masked"])
    assert torch.equal(out0["sop_logits"], out1["sop_logits"])
    total = math.sqrt(sum(float(g.norm()) ** 2 for g in g0.values()))
    worst = sorted(((float((g1[n] - g0[n]).norm()) / max(float(g0[n].norm()), 1e-5 * total), n) for n in g0), reverse=True)
    print("worst tensors", worst[:4])
    for r, n in worst:
        assert r < 3e-2, (n, r)
    for k in ev0:
        tol = slack * abs(float(ev0[k])) if "loss" in k else 0.0
        assert abs(float(ev0[k]) - float(ev1[k])) <= tol, (k, float(ev0[k]), float(ev1[k]))


@pytest.mark.parametrize("device", DEVICES, indirect=True)
def test_return_logits_and_encode_keep_their_contract(device, count_compact):
    m = _model(device)
    b = _batch(m.config.vocab_size, device, "positions")
    with torch.no_grad():
        h, Sp = m.encode(b["input_ids"], b["attention_mask"], b["token_type_ids"])
        assert h.shape == (B * S, m.config.hidden_size) and Sp == S and not count_compact
        out = m(b["input_ids"], b["attention_mask"], b["token_type_ids"], mlm_positions=b["mlm_positions"],
                mlm_labels=b["mlm_labels"], return_logits=True)
        assert len(count_compact) == 1
        assert out["prediction_logits_masked"].shape == (B * P, m.config.vocab_size)
        # the rows under the MLM head are the full output's rows
        ref = m._mlm_logits(h, (torch.arange(B, device=h.device)[:, None] * Sp + b["mlm_positions"]).reshape(-1))
        assert torch.equal(out["prediction_logits_masked"], ref)


@pytest.mark.parametrize("device", DEVICES, indirect=True)
def test_unsupported_combinations_run_the_full_layer(device, count_compact):
    b = None
    # head_dim 128: one head over the same hidden size
    m = _model(device, num_attention_heads=1)
    b = _batch(m.config.vocab_size, device, "positions")
    out, _ = _step(m, b)
    assert math.isfinite(float(out["loss"])) and not count_compact
    # a packed batch
    m = _model(device)
    out, _ = _step(m, b, pack_sequences=True, lengths=[S, 90, S])
    assert math.isfinite(float(out["loss"])) and not count_compact
    # a slot that would be no smaller than the sequence (1 + P rows round up to S' = 64)
    short = {k: (v[:, :64] if v.dim() == 2 and v.shape[1] == S else v) for k, v in b.items()}
    short["mlm_positions"] = short["mlm_positions"].clamp(max=63)
    out, _ = _step(m, short)
    assert math.isfinite(float(out["loss"])) and not count_compact
    # and the supported case does run it
    _step(m, b)
    assert len(count_compact) == 1
