"""ALBERT on packed, padding-free batches (``pack_sequences``) on the GPU.

Follows ``_compare`` of tests/test_albert_model.py: loss and flat gradient against HF
``transformers`` in fp32 with its bounds (loss_rtol 1e-2, grad_rtol 3e-2, the same per-tensor
rule), for a head_dim-64 and a head_dim-128 model and both MLM label forms; the packed and the
padded run of the same batch agree on the loss within the same 1e-2; each fine-tuning head's
logits on real tokens agree with the padded path; one AlbertPeer micro-step plus an optimizer step
runs with --pack_sequences on ``length_mode="uniform"``."""
import functools
import math

import pytest
import torch

import dedloc_amd.ops  # noqa: F401

pytestmark = pytest.mark.gpu

B, S = 4, 256
LENS = [17, 64, 130, 256]
LOSS_RTOL, GRAD_RTOL = 1e-2, 3e-2


def _config(head_dim):
    from dedloc_amd.models.albert import AlbertConfig

    hidden = 2 * head_dim  # 2 heads: hidden 128 (head_dim 64) / 256 (head_dim 128)
    return AlbertConfig.tiny(hidden_size=hidden, num_attention_heads=2, intermediate_size=4 * hidden,
                             num_hidden_layers=2, max_position_embeddings=S, classifier_dropout_prob=0.0)


def _batch(V, device, seed=0):
    from dedloc_amd.data.sop_dataset import mlm_targets

    g = torch.Generator().manual_seed(seed)
    am = (torch.arange(S)[None, :] < torch.tensor(LENS)[:, None]).long()
    ids = torch.randint(5, V, (B, S), generator=g) * am
    ids[:, 0] = 2
    tt = (torch.arange(S)[None, :] >= torch.tensor(LENS)[:, None] // 3).long() * am
    sel = (torch.rand(B, S, generator=g) < 0.15) & am.bool()
    sel[:, 0] = False
    sel[:, 1] = True  # every row has a target (its length permitting)
    sel &= am.bool()
    labels = torch.where(sel, torch.randint(5, V, (B, S), generator=g), torch.full((B, S), -100))
    sol = torch.randint(0, 2, (B,), generator=g)
    t = mlm_targets(sel, labels)  # the fixed-shape form of the same targets
    b = dict(ids=ids, am=am, tt=tt, labels=labels, sol=sol, pos=t["mlm_positions"], plab=t["mlm_labels"])
    return {k: v.to(device) for k, v in b.items()}


@functools.lru_cache(maxsize=None)
def _reference(head_dim):
    """Computed once per config and shared: our model, the fp32 HF gradients and loss, and the
    padded run of our model on the same batch."""
    import transformers

    from dedloc_amd.models.albert import AlbertForPreTraining

    dev = torch.device("cuda", 0)
    cfg = _config(head_dim)
    torch.manual_seed(0)
    ours = AlbertForPreTraining(cfg)
    sd = {k: v.detach().clone().float() for k, v in ours.hf_state_dict().items()}
    ours.materialize(dev)
    ours.eval()
    hcfg = transformers.AlbertConfig(**{k: v for k, v in cfg.to_dict().items() if k not in ("architectures", "model_type")})
    hcfg._attn_implementation = "eager"
    hf = transformers.AlbertForPreTraining(hcfg).to(dev).float().eval()
    missing, unexpected = hf.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    b = _batch(cfg.vocab_size, dev)
    ref = hf(input_ids=b["ids"], attention_mask=b["am"], token_type_ids=b["tt"], labels=b["labels"],
             sentence_order_label=b["sol"])
    ref.loss.backward()
    hf_grads = {k: (p.grad.float().clone() if p.grad is not None else None) for k, p in hf.named_parameters()}
    ours.flat.zero_grad()
    out = ours(b["ids"], b["am"], b["tt"], labels=b["labels"], sentence_order_label=b["sol"])
    out["loss"].backward()
    padded = (float(out["loss"].detach()), ours.flat.grad.detach().clone())
    ours.flat.zero_grad()
    return ours, b, float(ref.loss.detach()), hf_grads, padded


@pytest.mark.parametrize("form", ["labels", "positions"])
@pytest.mark.parametrize("head_dim", [64, 128])
def test_packed_loss_and_gradients_match_hf_fp32(cuda, head_dim, form):
    ours, b, l_ref, hf_grads, (l_pad, g_pad) = _reference(head_dim)
    kw = {"labels": b["labels"]} if form == "labels" else {"mlm_positions": b["pos"], "mlm_labels": b["plab"]}
    ours.flat.zero_grad()
    out = ours(b["ids"], b["am"], b["tt"], sentence_order_label=b["sol"], pack_sequences=True, lengths=LENS, **kw)
    out["loss"].backward()
    l_ours = float(out["loss"].detach())
    errs, num, den = {}, 0.0, 0.0
    for name in ours.flat.names:
        g_ours = ours.flat.g(name).float()
        g_ref = hf_grads[name] if hf_grads[name] is not None else torch.zeros_like(g_ours)
        d, n = (g_ours - g_ref).norm().item(), g_ref.norm().item()
        num += d * d
        den += n * n
        errs[name] = (d, n)
    total = math.sqrt(num) / math.sqrt(den)
    floor = 1e-5 * math.sqrt(den)
    rel = sorted(((d / max(n, floor), k) for k, (d, n) in errs.items()), reverse=True)
    vs_padded = ((ours.flat.grad - g_pad).norm() / g_pad.norm()).item()
    print(f"head_dim {head_dim} [{form}]: loss packed {l_ours:.5f} padded {l_pad:.5f} hf {l_ref:.5f}; flat-gradient "
          f"rel err vs hf {total:.2e}, vs padded {vs_padded:.2e}; worst tensors {rel[:3]}")
    ours.flat.zero_grad()
    assert abs(l_ours - l_ref) <= LOSS_RTOL * abs(l_ref), (l_ours, l_ref)
    assert abs(l_ours - l_pad) <= LOSS_RTOL * abs(l_pad), (l_ours, l_pad)  # packed vs padded, same batch
    assert total < GRAD_RTOL, (total, rel[:5])
    for r, k in rel:  # the per-tensor rule of tests/test_albert_model.py
        big = ours.flat.g(k).numel() >= 65536
        assert r < (GRAD_RTOL if big else 0.1), (k, r)


def _head_logits(cls, cuda, token_level):
    """Packed vs padded logits of a fine-tuning head on the real tokens.  Both paths run the same
    kernels on the same rows; what may differ is the GEMM tiling a different row count selects, i.e.
    bf16 rounding of intermediate activations (2^-8 = 3.9e-3 relative per rounding).  Bound: 1e-2 of
    the logits' norm, the loss tolerance above."""
    torch.manual_seed(0)
    m = cls(_config(64), num_labels=5)
    m.materialize(cuda)
    m.eval()
    b = _batch(m.config.vocab_size, cuda, seed=3)
    with torch.no_grad():
        pad = m(b["ids"], b["am"], b["tt"])["logits"].float()
        pk = m(b["ids"], b["am"], b["tt"], pack_sequences=True)["logits"].float()  # lengths from the mask
    assert pk.shape == pad.shape
    if token_level:
        real = b["am"].bool()
        pad, pk = pad[real], pk[real]
    err = ((pk - pad).norm() / pad.norm()).item()
    print(f"{cls.__name__}: packed vs padded logits rel err {err:.3e}")
    assert torch.isfinite(pk).all() and err < 1e-2, err


def test_sequence_classification_logits_match_padded(cuda):
    from dedloc_amd.models.albert import AlbertForSequenceClassification

    _head_logits(AlbertForSequenceClassification, cuda, False)


def test_token_classification_logits_match_padded(cuda):
    from dedloc_amd.models.albert import AlbertForTokenClassification

    _head_logits(AlbertForTokenClassification, cuda, True)


def test_peer_microstep_with_pack_sequences(cuda, tmp_path):
    from dedloc_amd.cli.arguments import AlbertTrainingArguments, CollaborationArguments, DatasetArguments
    from dedloc_amd.dht import DHT
    from dedloc_amd.training.albert_peer import AlbertPeer

    cfg = tmp_path / "cfg"
    _config(64).save_pretrained(str(cfg))
    root = DHT(listen_on="127.0.0.1:*")
    peer = None
    try:
        targs = AlbertTrainingArguments(per_device_train_batch_size=8, gradient_accumulation_steps=1, seq_length=S,
                                        save_steps=0, output_dir=str(tmp_path / "out"), seed=0, pack_sequences=True)
        cargs = CollaborationArguments(experiment_prefix="packed", initial_peers=[root.endpoint],
                                       dht_listen_on="127.0.0.1:*", target_batch_size=4096, listen_on="127.0.0.1:*")
        peer = AlbertPeer(targs, DatasetArguments(config_path=str(cfg), length_mode="uniform"), cargs, cuda)
        assert peer.model.pack_sequences
        seen = []  # the loss of the peer's own forward call (the peer folds it into its metrics at once)
        hook = peer.model.register_forward_hook(lambda mod, args, out: seen.append(out["loss"].detach()))
        peer.train_step()  # one micro-step through the peer: packed forward / backward, clip, accumulate
        hook.remove()
        assert peer.data.last_lengths is not None and min(peer.data.last_lengths) < S  # host lengths, short rows
        loss, (gnorm, finite) = float(seen[0]), peer._clip_out[:2].tolist()
        print(f"peer micro-step: loss {loss:.4f} grad norm {gnorm:.4f}")
        assert math.isfinite(loss) and loss > 0 and math.isfinite(gnorm) and gnorm > 0 and finite == 1.0
        # and an optimizer step on a packed micro-step's gradient
        b = peer.data.next_batch()
        out = peer.model(b["input_ids"], b["attention_mask"], b["token_type_ids"],
                         sentence_order_label=b["sentence_order_label"], mlm_positions=b["mlm_positions"],
                         mlm_labels=b["mlm_labels"], lengths=peer.data.last_lengths)
        out["loss"].backward()
        assert torch.isfinite(peer.model.flat.grad).all()
        peer.opt.step()
        assert torch.isfinite(peer.model.flat.fp32).all() and math.isfinite(float(out["loss"].detach()))
    finally:
        if peer is not None:
            peer.shutdown()
        root.shutdown()
