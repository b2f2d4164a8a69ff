"""AlbertForPreTraining on a packed batch with its last layer on the rows the heads read
(``last_layer_rows=True``) against the full last layer on the same packed batch, CPU ops and GPU.
Tiny config, S = 1024, lengths [S, 90, S, 40]: slots of 1024, 128, 1024, 64 rows and, at 2240 rows, a
dummy tail of 64.  Sequence 0 carries 66 MLM targets, so Sq = 128 exceeds the slot of the 40-token
sequence; sequence 2 has none.  Bounds: tests/test_albert_last_layer_rows.py (losses within the
reordering slack of the kernels' atomic loss sum, 64 * 2^-24 on the GPU and 0 on the CPU; every
gradient tensor within 3e-2 of its norm, floored at 1e-5 of the total; evaluate_batch equal)."""
import math

import pytest
import torch

import dedloc_amd.models.albert as albert
from test_albert_last_layer_rows import DEVICES, _model, _step, device  # noqa: F401  (device: fixture)

S, P = 1024, 70
LENS = [S, 90, S, 40]
TARGETS = [66, 3, 0, 2]  # MLM targets per sequence
PACKED = dict(pack_sequences=True, lengths=LENS)


def _batch(V, device, form):
    g = torch.Generator().manual_seed(1)
    B = len(LENS)
    am = (torch.arange(S)[None, :] < torch.tensor(LENS)[:, None]).long()
    ids = torch.randint(5, V, (B, S), generator=g) * am
    tt = (torch.arange(S)[None, :] >= torch.tensor(LENS)[:, None] // 3).long() * am
    batch = {"input_ids": ids, "attention_mask": am, "token_type_ids": tt,
             "sentence_order_label": torch.randint(0, 2, (B,), generator=g)}
    pos = torch.zeros(B, P, dtype=torch.long)  # unused entries: position 0, label -100
    lab = torch.full((B, P), -100, dtype=torch.long)
    labels = torch.full((B, S), -100, dtype=torch.long)
    for b, n in enumerate(TARGETS):
        pos[b, :n] = torch.randperm(LENS[b] - 1, generator=g)[:n].sort().values + 1
        lab[b, :n] = torch.randint(5, V, (n,), generator=g)
        labels[b, pos[b, :n]] = lab[b, :n]
    batch.update({"labels": labels} if form == "labels" else {"mlm_positions": pos, "mlm_labels": lab})
    return {k: v.to(device) for k, v in batch.items()}


@pytest.mark.parametrize("device", DEVICES, indirect=True)
@pytest.mark.parametrize("form", ["labels", "positions"])
def test_packed_last_layer_rows_match_full_last_layer(device, form, monkeypatch):
    calls, real = [], albert.ops.attn_varlen_fwd_q  # calls: the Sq of every compact attention call
    monkeypatch.setattr(albert.ops, "attn_varlen_fwd_q", lambda *a, **k: (calls.append(a[6]), real(*a, **k))[1])
    m = _model(device, max_position_embeddings=S)  # eval mode: no classifier dropout
    m.pack_sequences = True  # evaluate_batch reads the attribute
    b = _batch(m.config.vocab_size, device, form)
    _step(m, b, **PACKED)  # the default: the full layer
    out0, g0 = _step(m, b, last_layer_rows=False, **PACKED)
    ev0 = m.evaluate_batch(b, lengths=LENS, last_layer_rows=False)
    assert not calls
    out1, g1 = _step(m, b, last_layer_rows=True, **PACKED)
    ev1 = m.evaluate_batch(b, lengths=LENS, last_layer_rows=True)
    assert calls == [128, 128]  # forward and evaluate_batch; Sq beyond the 64-row slot of sequence 3
    slack = 64 * 2.0 ** -24 if device.type == "cuda" else 0.0
    for k in ("loss", "mlm_loss", "sop_loss"):
        a, c = float(out0[k].detach()), float(out1[k].detach())
        print(k, a, c)
        assert math.isfinite(c) and abs(a - c) <= slack * abs(a), k
    total = math.sqrt(sum(float(g.norm()) ** 2 for g in g0.values()))
    worst = sorted(((float((g1[n] - g0[n]).norm()) / max(float(g0[n].norm()), 1e-5 * total), n) for n in g0), reverse=True)
    print("worst tensors", worst[:4])
    assert worst[0][0] < 3e-2, worst[0]
    for k in ev0:
        tol = slack * abs(float(ev0[k])) if "loss" in k else 0.0
        assert abs(float(ev0[k]) - float(ev1[k])) <= tol, (k, float(ev0[k]), float(ev1[k]))
