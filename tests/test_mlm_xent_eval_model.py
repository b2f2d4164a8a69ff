"""``evaluate_batch`` on the fused MLM evaluation (``_FUSED_MLM_EVAL``) against the decoder GEMM +
``ops.eval_cross_entropy`` path it replaces, and the CPU implementation of ``ops.mlm_eval_cross_entropy``."""
import pytest
import torch

import dedloc_amd.ops as ops


def test_cpu_matches_eval_cross_entropy_on_fp32_logits():
    """Integer-valued inputs (every fp32 score exact, ties frequent): the op equals
    ``eval_cross_entropy`` on the unrounded logits, so it shares its tie rule."""
    g = torch.Generator().manual_seed(7)
    t, w = (torch.randint(-2, 3, (m, 128), generator=g).bfloat16() for m in (65, 200))
    bias = torch.randint(-4, 5, (200,), generator=g) * 0.5
    w[[0, 99, 101, 199]], bias[[0, 99, 101, 199]] = w[100].clone(), bias[100].clone()
    x = t.float() @ w.float().t() + bias
    labels = torch.randint(0, 200, (65,), generator=g)
    labels[4::5] = x.argmax(1)[4::5]
    labels[0::5], labels[1::5], labels[3::5], labels[2::4] = 100, 0, 199, -100
    y = labels.clamp(min=0)[:, None]
    rank = ((x > x.gather(1, y)) | ((x == x.gather(1, y)) & (torch.arange(200)[None, :] < y))).sum(1)[labels != -100]
    got, want = ops.mlm_eval_cross_entropy(t, w, bias, labels), ops.eval_cross_entropy(x, labels)
    assert all(torch.equal(got[k], want[k]) for k in ("loss_sum", "count", "top1", "top5"))
    assert (int(got["count"]), int(got["top1"]), int(got["top5"])) == (len(rank), int((rank == 0).sum()), int((rank < 5).sum()))
    assert 0 < int(got["top1"]) <= int(got["top5"]) < int(got["count"])


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [False, True])
def test_evaluate_batch_switch(cuda, monkeypatch, packed):
    from dedloc_amd.data.synthetic_mlm import SyntheticSOPStream
    from dedloc_amd.models import albert

    torch.manual_seed(0)
    model = albert.AlbertForPreTraining(albert.AlbertConfig.tiny(num_hidden_layers=2, max_position_embeddings=64,
                                                                 embedding_size=128))
    model.materialize(cuda)
    model.pack_sequences = packed
    stream = SyntheticSOPStream(8, 64, 512, seed=3, device="cpu", mask_mode="hf", length_mode="uniform", min_len=9)
    batch = {k: v.to(cuda) for k, v in stream.next_batch().items()}
    lengths = stream.last_lengths if packed else None
    calls, logits_fn = [], model._mlm_logits
    monkeypatch.setattr(model, "_mlm_logits", lambda h, rows: calls.append(1) or logits_fn(h, rows))
    fused = model.evaluate_batch(batch, lengths=lengths)
    assert not calls  # the fused path never forms the logits
    monkeypatch.setattr(albert, "_FUSED_MLM_EVAL", False)
    plain = model.evaluate_batch(batch, lengths=lengths)
    assert len(calls) == 1
    for k in ("mlm_count", "sop_loss_sum", "sop_count", "sop_correct"):
        assert torch.equal(fused[k], plain[k]), k
    assert float(fused["mlm_loss_sum"]) == pytest.approx(float(plain["mlm_loss_sum"]), rel=1e-2)
    # bf16 rounding keeps the order of two fp32 logits or ties them: only rows whose label ties in
    # the bf16 logits can rank differently on the fp32 scores
    model.eval()
    with torch.no_grad():
        x = model(batch["input_ids"], batch["attention_mask"], batch["token_type_ids"], labels=batch["labels"],
                  return_logits=True, lengths=lengths)["prediction_logits_masked"]
    tgt = batch["labels"][batch["labels"] != -100]
    ties = int(((x == x.gather(1, tgt[:, None])).sum(1) > 1).sum())
    for k in ("mlm_top1", "mlm_top5"):
        assert abs(int(fused[k]) - int(plain[k])) <= ties, (k, int(fused[k]), int(plain[k]), ties)
