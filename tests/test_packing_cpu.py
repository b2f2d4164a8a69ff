"""Padding-free batches on the CPU tier: the packing helpers (data/packing.py), the CPU
implementations of the packed ops against the existing ops run sequence by sequence, and a tiny
ALBERT packed vs padded for all three model classes."""
import math

import pytest
import torch

import dedloc_amd.ops as ops  # noqa: F401  (registers the dedloc:: operators)
from dedloc_amd.data.packing import pack_batch, slot_rows, unpack_rows
from dedloc_amd.data.synthetic_mlm import SyntheticSOPStream
from dedloc_amd.models.albert import (AlbertConfig, AlbertForPreTraining, AlbertForSequenceClassification,
                                      AlbertForTokenClassification)

OPS = torch.ops.dedloc
LENS = [1, 63, 64, 65, 128, 100]
S = 128


def _batch(lens=LENS, S=S, seed=0, vocab=500, labels=True):
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    am = (torch.arange(S)[None, :] < torch.tensor(lens)[:, None]).long()
    ids = torch.randint(5, vocab, (B, S), generator=g) * am
    tt = ((torch.arange(S)[None, :] >= torch.tensor(lens)[:, None] // 2) & am.bool()).long()
    b = {"input_ids": ids, "token_type_ids": tt, "attention_mask": am}
    if labels:
        pick = (torch.rand(B, S, generator=g) < 0.3) & am.bool()
        pick[:, 0] = True  # every row has a target
        b["labels"] = torch.where(pick, ids, torch.full_like(ids, -100))
    return b


# ------------------------------------------------------------------ pack_batch / unpack_rows
def test_pack_layout_and_filler():
    b = _batch()
    pk = pack_batch(b, LENS, pad_token_id=0)
    rows = slot_rows(LENS)
    assert rows == [0, 64, 128, 192, 320, 448, 576] and pk.rows == rows
    assert pk.T == 576 and pk.max_slot == 128 and pk.B == len(LENS) and pk.real_tokens == sum(LENS)
    assert pk.seqinfo_host.dtype == torch.int32 and pk.seqinfo_host.tolist() == rows + LENS
    assert torch.equal(pk.seqinfo.cpu(), pk.seqinfo_host) and pk.n_seq == pk.B  # 576 rows need no tail
    for i, n in enumerate(LENS):
        r0, r1 = rows[i], rows[i + 1]
        assert r0 % 64 == 0 and r1 - r0 == (n + 63) // 64 * 64
        # real rows: the sequence's tokens, in order
        assert torch.equal(pk.input_ids[r0:r0 + n], b["input_ids"][i, :n])
        assert torch.equal(pk.token_type_ids[r0:r0 + n], b["token_type_ids"][i, :n])
        assert torch.equal(pk.extras["labels"][r0:r0 + n], b["labels"][i, :n])
        # positions continue through the filler; filler = pad id, type 0, no labels
        assert pk.positions[r0:r1].tolist() == list(range(r1 - r0))
        assert (pk.input_ids[r0 + n:r1] == 0).all() and (pk.token_type_ids[r0 + n:r1] == 0).all()
        assert (pk.extras["labels"][r0 + n:r1] == -100).all()
        assert pk.real[r0:r0 + n].all() and not pk.real[r0 + n:r1].any()


def test_dummy_tail_sequence():
    """T is rounded up to tail_granule(T) rows by one dummy sequence of pad tokens whose key length
    is its own slot size; it has no real row, no label, and positions inside the table."""
    from dedloc_amd.data.packing import tail_granule

    assert [tail_granule(t) for t in (64, 576, 2047, 2048, 5248, 16384, 32768, 10 ** 6)] == \
        [64, 64, 64, 128, 256, 1024, 1024, 1024]
    from dedloc_amd.data.packing import make_seqinfo

    # a tail longer than the largest real slot is split, so the attention grids do not grow
    _, host, rows, ls = make_seqinfo([512] * 37 + [70], "cpu")  # 19072 rows -> 19456: 384 more
    assert rows[-1] == 19456 and ls[38:] == [384]
    _, host, rows, ls = make_seqinfo([256] * 66 + [64], "cpu")   # 16960 rows -> 17408: 448 = 256 + 192
    assert rows[-1] == 17408 and ls[67:] == [256, 192] and host.tolist() == rows + ls
    lens = [128] * 40 + [100]          # 41 slots of 128 rows = 5248 rows -> granule 256 -> 5376 rows
    b = _batch(lens, seed=2)
    pk = pack_batch(b, lens, pad_token_id=0)
    assert pk.T == 5376 and pk.B == 41 and pk.n_seq == 42 and pk.max_slot == 128 and pk.lengths == lens
    si = pk.seqinfo_host.tolist()
    assert si[:43] == pk.rows and si[41] == 5248 and si[42] == 5376 and si[43:] == lens + [128]
    tail = slice(5248, 5376)
    assert not pk.real[tail].any() and (pk.input_ids[tail] == 0).all() and (pk.token_type_ids[tail] == 0).all()
    assert (pk.extras["labels"][tail] == -100).all() and int(pk.positions[tail].max()) < 64
    assert pk.row_start.tolist() == pk.rows[:41]
    x = torch.randn(41, S, 2)
    assert torch.equal(unpack_rows(pk.pack_tokens(x, 0.0), pk, S)[b["attention_mask"].bool()],
                       x[b["attention_mask"].bool()])
    # the packed ops accept it, and the dummy's rows come out finite
    H, D = 2, 64
    qkv = torch.randn(pk.T, 3 * H * D).bfloat16()
    out, lse = OPS.attn_varlen_fwd(qkv, pk.seqinfo, pk.seqinfo_host, H, 0.125)
    assert torch.isfinite(out[tail].float()).all() and torch.isfinite(lse[:, tail]).all()


def test_model_with_dummy_tail_equals_padded():
    """The dummy tail adds exactly nothing: loss and gradient of a packed batch that needs one
    against the padded run (bounds as in _compare below)."""
    m = _model(AlbertForPreTraining)
    lens = [128] * 40 + [100]
    b = _batch(lens, seed=4)
    sop = torch.arange(41) % 2
    res = _both(m, lambda pack: m(b["input_ids"], b["attention_mask"], b["token_type_ids"], labels=b["labels"],
                                  sentence_order_label=sop, pack_sequences=pack, lengths=lens if pack else None))
    _compare("pretraining with a dummy tail", res, rows=41 * 128)


def test_pad_token_id_is_used_for_filler():
    pk = pack_batch(_batch(), LENS, pad_token_id=7)
    assert (pk.input_ids[~pk.real] == 7).all()


def test_mask_lengths_equal_host_lengths():
    b = _batch()
    a, c = pack_batch(b, LENS), pack_batch(b)  # host lengths vs lengths read from the mask
    assert a.lengths == c.lengths and a.rows == c.rows and (a.T, a.max_slot) == (c.T, c.max_slot)
    for k in ("input_ids", "token_type_ids", "positions", "seqinfo", "seqinfo_host", "src", "real", "row_start"):
        assert torch.equal(getattr(a, k), getattr(c, k)), k
    assert torch.equal(a.extras["labels"], c.extras["labels"])


def test_non_prefix_mask_raises():
    b = _batch()
    b["attention_mask"][3, 5] = 0
    with pytest.raises(ValueError, match="prefix"):
        pack_batch(b)


def test_bad_lengths_raise():
    b = _batch()
    with pytest.raises(ValueError):
        pack_batch(b, [0] + LENS[1:])  # never a zero-length sequence
    with pytest.raises(ValueError):
        pack_batch(b, LENS[:-1] + [S + 1])
    with pytest.raises(ValueError):
        pack_batch(b, LENS[:-1])


def test_unpack_round_trip():
    b = _batch()
    pk = pack_batch(b, LENS)
    x = torch.randn(len(LENS), S, 3)
    am = b["attention_mask"].bool()
    back = unpack_rows(pk.pack_tokens(x, 0.0), pk, S)
    assert back.shape == x.shape
    assert torch.equal(back[am], x[am])  # real tokens survive the round trip
    assert (back[~am] == 0).all()        # filler rows were filled with 0, rows past a slot do not exist
    # a narrower view is a prefix of the wide one
    assert torch.equal(unpack_rows(pk.pack_tokens(x, 0.0), pk, 64), back[:, :64])
    # packed per-row values land at rows[b] + position
    t = torch.arange(pk.T).float()[:, None]
    u = unpack_rows(t, pk, S)
    for i, n in enumerate(LENS):
        assert u[i, :n, 0].tolist() == [float(pk.rows[i] + s) for s in range(n)]


def test_uniform_length_mode():
    st = SyntheticSOPStream(16, 128, 500, seed=3, length_mode="uniform", min_len=16)
    seen = []
    for _ in range(8):
        b = st.next_batch()
        lens = b["attention_mask"].sum(1).tolist()
        assert lens == st.last_lengths and all(16 <= n <= 128 for n in lens)
        seen += lens
    assert min(seen) < 40 and max(seen) > 100  # spread over the range, not clustered at S
    assert SyntheticSOPStream(4, 128, 500).next_batch()["attention_mask"].all()  # the default stays "full"
    with pytest.raises(ValueError):
        SyntheticSOPStream(4, 128, 500, length_mode="nope")


# ------------------------------------------------------------------ CPU ops vs the existing ops, per sequence
@pytest.mark.parametrize("D", [64, 128])
def test_cpu_attn_varlen_equals_per_sequence(D):
    torch.manual_seed(1)
    H = 2
    lens = [1, 63, 65, 128]
    pk = pack_batch(_batch(lens, labels=False), lens)
    scale = 1.0 / math.sqrt(D)
    qkv = torch.randn(pk.T, 3 * H * D).bfloat16()
    dout = torch.randn(pk.T, H * D).bfloat16()
    out, lse = OPS.attn_varlen_fwd(qkv, pk.seqinfo, pk.seqinfo_host, H, scale)
    db = torch.zeros(3 * H * D)
    dqkv = OPS.attn_varlen_bwd(qkv, pk.seqinfo, pk.seqinfo_host, out, dout, lse, H, scale, db)
    assert out.shape == (pk.T, H * D) and lse.shape == (H, pk.T)
    db_ref = torch.zeros_like(db)
    for i, n in enumerate(lens):
        r0, r1 = pk.rows[i], pk.rows[i + 1]
        mb = torch.where(torch.arange(r1 - r0) < n, 0.0, -1e30).float()[None, :]
        o, l = OPS.attn_fwd(qkv[r0:r1], mb, H, r1 - r0, scale, None)
        g = OPS.attn_bwd(qkv[r0:r1], mb, o, dout[r0:r1], l, H, r1 - r0, scale, None, db_ref)
        assert torch.equal(out[r0:r1], o) and torch.equal(lse[:, r0:r1], l[0]) and torch.equal(dqkv[r0:r1], g)
        assert dqkv[r0 + n:r1, H * D:].abs().max().item() == 0.0 if n < r1 - r0 else True
    assert torch.allclose(db, db_ref, rtol=1e-6, atol=1e-6)


def test_cpu_packed_ops_refuse_contract_violations():
    H, D = 2, 64
    qkv = torch.randn(128, 3 * H * D).bfloat16()

    def call(rows, lens, q=qkv):
        si = torch.tensor(rows + lens, dtype=torch.int32)
        return OPS.attn_varlen_fwd(q, si, si, H, 0.125)

    for rows, lens in (([0, 96, 128], [50, 30]), ([0, 64, 128], [0, 60]), ([0, 64, 128], [64, 65])):
        with pytest.raises(RuntimeError):
            call(rows, lens)
    with pytest.raises(RuntimeError, match="supported head sizes are 64 and 128"):
        call([0, 64, 128], [64, 64], torch.randn(128, 3 * H * 32).bfloat16())


def test_cpu_packed_embedding_equals_per_sequence():
    torch.manual_seed(2)
    E, V = 64, 500
    b = _batch(labels=False)
    pk = pack_batch(b, LENS)
    wemb, pemb, temb = torch.randn(V, E), torch.randn(S, E), torch.randn(2, E)
    gamma, beta = torch.rand(E) + 0.5, torch.randn(E)
    y, s, mean, rstd = OPS.embed_ln_pos_fwd(pk.input_ids, pk.token_type_ids, pk.positions, wemb, pemb, temb, gamma,
                                            beta, 1e-12)
    ds = torch.randn(pk.T, E).bfloat16()
    gw, gp, gt = torch.zeros(V, E), torch.zeros(S, E), torch.zeros(2, E)
    OPS.embed_pos_bwd(ds, pk.input_ids, pk.token_type_ids, pk.positions, gw, gp, gt)
    rw, rp, rt = torch.zeros(V, E), torch.zeros(S, E), torch.zeros(2, E)
    for i in range(len(LENS)):
        r0, r1 = pk.rows[i], pk.rows[i + 1]  # one slot = one sequence of r1 - r0 positions for the existing op
        y1, s1, m1, q1 = OPS.embed_ln_fwd(pk.input_ids[r0:r1], pk.token_type_ids[r0:r1], wemb, pemb, temb, gamma, beta,
                                          r1 - r0, 1e-12)
        assert torch.equal(y[r0:r1], y1) and torch.equal(s[r0:r1], s1)
        assert torch.equal(mean[r0:r1], m1) and torch.equal(rstd[r0:r1], q1)
        OPS.embed_bwd(ds[r0:r1], pk.input_ids[r0:r1], pk.token_type_ids[r0:r1], rw, rp, rt, r1 - r0)
    for a, r in ((gw, rw), (gp, rp), (gt, rt)):
        assert torch.allclose(a, r, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------ tiny ALBERT, packed vs padded
MODEL_LENS = [17, 64, 100, 128]


def _model(cls, **kw):
    torch.manual_seed(0)
    m = cls(AlbertConfig.tiny(classifier_dropout_prob=0.0), **kw)
    m.materialize("cpu")
    m.train()
    return m


def _both(model, call):
    res = []
    for pack in (False, True):
        model.flat.grad.zero_()
        out = call(pack)
        out["loss"].backward()
        res.append((out, model.flat.grad.clone()))
    return res


def _compare(case, res, rows=512):
    """Same loss to 1e-5 relative and a flat gradient equal to within fp32 summation noise.

    The two runs execute the same per-row arithmetic (bf16 activations, fp32 accumulation); only
    the order in which rows are summed into each weight gradient differs (T packed rows instead of
    B*S' padded ones, zero rows dropped).  Reordering an fp32 sum of n terms moves it by at most
    ~n * 2^-24 relative to the sum of magnitudes; with n <= 512 rows here that is 3e-5, so the bound
    on |g_packed - g_padded| / |g_padded| is 1e-4 (scaled with the row count for the one larger
    case).  Measured: 8e-8 .. 2.3e-7 (printed below)."""
    (o0, g0), (o1, g1) = res
    l0, l1 = float(o0["loss"].detach()), float(o1["loss"].detach())
    gdiff = ((g1 - g0).norm() / g0.norm()).item()
    print(f"{case}: loss padded {l0:.7f} packed {l1:.7f}; |dg|/|g| = {gdiff:.3e}")
    assert abs(l1 - l0) <= 1e-5 * abs(l0), (l0, l1)
    assert torch.isfinite(g1).all() and gdiff < 1e-4 * max(1, rows / 512), gdiff
    return o0, o1


@pytest.mark.parametrize("form", ["labels", "positions"])
def test_pretraining_packed_equals_padded(form):
    m = _model(AlbertForPreTraining)
    b = _batch(MODEL_LENS, seed=5)
    sop = torch.tensor([0, 1, 1, 0])
    kw = {"labels": b["labels"]}
    if form == "positions":
        P = 8
        pos = torch.stack([torch.randperm(n, generator=torch.Generator().manual_seed(n))[:P] if n >= P else
                           torch.arange(P) % n for n in MODEL_LENS])
        lab = torch.gather(b["input_ids"], 1, pos)
        lab[0, 4:] = -100  # padded target slots
        kw = {"mlm_positions": pos, "mlm_labels": lab}
    res = _both(m, lambda pack: m(b["input_ids"], b["attention_mask"], b["token_type_ids"], sentence_order_label=sop,
                                  return_logits=True, pack_sequences=pack,
                                  lengths=MODEL_LENS if pack else None, **kw))
    o0, o1 = _compare(f"pretraining[{form}]", res)
    assert set(o0) == set(o1)
    assert torch.allclose(o1["prediction_logits_masked"].float(), o0["prediction_logits_masked"].float(), atol=1e-6)
    assert torch.allclose(o1["sop_logits"].float(), o0["sop_logits"].float(), atol=1e-6)


def test_sequence_classification_packed_equals_padded():
    m = _model(AlbertForSequenceClassification, num_labels=3)
    b = _batch(MODEL_LENS, seed=6, labels=False)
    y = torch.tensor([0, 2, 1, 1])
    m.pack_sequences = True  # the trainer's way: the attribute, lengths read from the mask
    res = _both(m, lambda pack: m(b["input_ids"], b["attention_mask"], labels=y, pack_sequences=pack))
    o0, o1 = _compare("sequence_classification", res)
    assert torch.allclose(o1["logits"].float(), o0["logits"].float(), atol=1e-6)


def test_token_classification_packed_equals_padded():
    m = _model(AlbertForTokenClassification, num_labels=5)
    b = _batch(MODEL_LENS, seed=7, labels=False)
    am = b["attention_mask"].bool()
    y = torch.where(am, torch.randint(0, 5, am.shape, generator=torch.Generator().manual_seed(1)), -100)
    res = _both(m, lambda pack: m(b["input_ids"], b["attention_mask"], b["token_type_ids"], labels=y,
                                  pack_sequences=pack))
    o0, o1 = _compare("token_classification", res)
    assert o1["logits"].shape == o0["logits"].shape == (4, S, 5)  # returned unpacked
    assert torch.allclose(o1["logits"][am].float(), o0["logits"][am].float(), atol=1e-6)


def test_packed_mode_refuses_other_head_sizes():
    torch.manual_seed(0)
    m = AlbertForSequenceClassification(AlbertConfig.tiny(num_attention_heads=4), num_labels=2)  # head_dim 32
    m.materialize("cpu")
    b = _batch(MODEL_LENS, labels=False)
    with pytest.raises(RuntimeError, match="head_dim 32"):
        m(b["input_ids"], b["attention_mask"], pack_sequences=True)
    m(b["input_ids"], b["attention_mask"])  # the rectangular path still serves it


# ------------------------------------------------------------------ the flag on the entry points
def test_contributor_passes_pack_sequences_to_run_trainer(capsys):
    import json

    from transformers import HfArgumentParser

    from dedloc_amd.cli.arguments import AlbertTrainingArguments, CollaborationArguments, DatasetArguments
    from dedloc_amd.cli.contributor import main

    parser = HfArgumentParser((AlbertTrainingArguments, DatasetArguments, CollaborationArguments))
    for flags, want in ((["--pack_sequences"], True), ([], False)):
        main(["--device", "cpu", "--dry_run", *flags])
        argv = json.loads(capsys.readouterr().out)["run_trainer"]
        t, _, _ = parser.parse_args_into_dataclasses(argv[1:])  # argv[0] is --sahajbert (run_trainer's own)
        assert t.pack_sequences is want


@pytest.mark.parametrize("task", ["ner", "ncc"])
def test_finetune_with_pack_sequences(task):
    """One epoch of cli/finetune.py with and without --pack_sequences at 128 tokens (rows of 64 .. 127
    tokens, so slots of 64 and 128 rows).  ncc: the only dropout acts on the pooled [B, hidden]
    tensor, the same shape in both layouts, so the two runs draw the same masks and differ by fp32
    summation order only: evaluation losses agree to 1e-4 relative.  ner: token dropout acts on
    [T, hidden] instead of [B * S', hidden], the runs draw different masks, and only a finite loss of
    the usual size is asserted."""
    from dedloc_amd.cli import finetune

    res = []
    for extra in ([], ["--pack_sequences"]):
        args = finetune.parse_args(["--task", task, "--train_samples", "16", "--eval_samples", "8",
                                    "--per_device_train_batch_size", "8", "--num_train_epochs", "1",
                                    "--max_seq_length", "128", "--learning_rate", "1e-3", *extra])
        res.append(finetune.run(args)["history"][0]["eval_loss"])
    print(f"finetune {task}: eval loss padded {res[0]:.6f} packed {res[1]:.6f}")
    assert math.isfinite(res[1]) and 0 < res[1] < 2 * res[0]
    if task == "ncc":
        assert abs(res[1] - res[0]) <= 1e-4 * abs(res[0]), res
