"""Local evaluation (``--do_eval``): ``AlbertForPreTraining.evaluate_batch``, ``training/evaluation.py``,
the peer loop and the coordinator, on the tiny config; one GPU test against the CPU result."""
import importlib.util
import json
import math
import os

import pytest
import torch

import dedloc_amd.ops  # noqa: F401
from conftest import record_margin

_spec = importlib.util.spec_from_file_location(
    "_xent_eval_oracle", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_xent_eval_cpu.py"))
_cpu = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_cpu)
oracle = _cpu.oracle

SUMS = ("mlm_loss_sum", "mlm_count", "mlm_top1", "mlm_top5", "sop_loss_sum", "sop_count", "sop_correct")
EVAL_KEYS = {"eval_loss", "eval_mlm_loss", "eval_sop_loss", "eval_mlm_accuracy", "eval_mlm_top5", "eval_sop_accuracy",
             "eval_perplexity", "eval_samples"}


def _tiny(device="cpu", seed=0, **kw):
    from dedloc_amd.models.albert import AlbertConfig, AlbertForPreTraining

    torch.manual_seed(seed)
    model = AlbertForPreTraining(AlbertConfig.tiny(num_hidden_layers=2, max_position_embeddings=64, **kw))
    model.materialize(torch.device(device))
    return model


def _stream(mask_mode, device="cpu", seed=3, B=4, **kw):
    from dedloc_amd.data.synthetic_mlm import SyntheticSOPStream

    return SyntheticSOPStream(B, 64, 512, seed=seed, device=device, mask_mode=mask_mode, **kw)


def _form(batch, form):
    """The batch with one MLM target form only: HF ``labels`` or ``mlm_positions``/``mlm_labels``."""
    drop = ("mlm_positions", "mlm_labels") if form == "labels" else ("labels",)
    return {k: v for k, v in batch.items() if k not in drop}


def _expected(model, batch):
    """evaluate_batch's sums derived from forward(..., return_logits=True) in eval mode and the oracle."""
    was = model.training
    model.eval()
    with torch.no_grad():
        out = model(batch["input_ids"], batch["attention_mask"], batch["token_type_ids"], labels=batch.get("labels"),
                    sentence_order_label=batch["sentence_order_label"], mlm_positions=batch.get("mlm_positions"),
                    mlm_labels=batch.get("mlm_labels"), return_logits=True)
    model.train(was)
    if "mlm_positions" in batch:
        tgt = batch["mlm_labels"].reshape(-1)
    else:
        tgt = batch["labels"].reshape(-1)
        tgt = tgt[tgt != -100]
    ml, mr = oracle(out["prediction_logits_masked"], tgt)
    sl, sr = oracle(out["sop_logits"], batch["sentence_order_label"])
    return {"mlm_loss_sum": float(ml.double().sum()), "mlm_count": int((mr >= 0).sum()),
            "mlm_top1": int((mr == 0).sum()), "mlm_top5": int(((mr >= 0) & (mr < 5)).sum()),
            "sop_loss_sum": float(sl.double().sum()), "sop_count": int((sr >= 0).sum()),
            "sop_correct": int((sr == 0).sum())}, out


@pytest.mark.parametrize("form,mask_mode", [("labels", "hf"), ("positions", "hf"), ("positions", "fixed")])
def test_evaluate_batch_matches_forward_and_oracle(form, mask_mode):
    model = _tiny()
    model.train()
    batch = _form(_stream(mask_mode).next_batch(), form)
    with torch.no_grad():
        model.flat.grad.copy_(torch.randn(model.flat.grad.shape, generator=torch.Generator().manual_seed(1)))
    grad0 = model.flat.grad.clone()
    rng0 = torch.get_rng_state()
    got = model.evaluate_batch(batch)
    assert torch.equal(torch.get_rng_state(), rng0)
    assert model.training  # the previous mode is back
    assert torch.equal(model.flat.grad.view(torch.int32), grad0.view(torch.int32))  # bit-unchanged
    assert set(got) == set(SUMS) and all(isinstance(v, torch.Tensor) and v.dim() == 0 for v in got.values())
    want, out = _expected(model, batch)
    assert want["mlm_count"] > 0 and want["sop_count"] == 4
    for k in SUMS:
        if k.endswith("loss_sum"):
            assert float(got[k]) == pytest.approx(want[k], rel=1e-5), k
        else:
            assert int(got[k]) == want[k], k
    # the means are forward's losses
    assert float(got["mlm_loss_sum"]) / want["mlm_count"] == pytest.approx(float(out["mlm_loss"]), rel=1e-5)
    assert float(got["sop_loss_sum"]) / want["sop_count"] == pytest.approx(float(out["sop_loss"]), rel=1e-5)
    model.eval()
    model.evaluate_batch(batch)
    assert not model.training


@pytest.mark.parametrize("form", ["labels", "positions"])
def test_evaluate_batch_packed_cpu(form):
    """pack_sequences takes the packed encoder path: same rows under the heads, so exact counts; the
    losses within the 1e-2 that tests/test_albert_packed_gpu.py allows between packed and padded."""
    model = _tiny()
    stream = _stream("hf", length_mode="uniform", min_len=9)
    batch = _form(stream.next_batch(), form)
    rect = model.evaluate_batch(batch)
    model.pack_sequences = True
    packed = model.evaluate_batch(batch, lengths=stream.last_lengths)
    nolen = model.evaluate_batch(batch)
    for k in ("mlm_count", "sop_count"):
        assert int(packed[k]) == int(rect[k]) == int(nolen[k])
    for k in ("mlm_loss_sum", "sop_loss_sum"):
        assert float(packed[k]) == pytest.approx(float(rect[k]), rel=1e-2)
        assert torch.equal(packed[k], nolen[k])


def test_evaluation_leaves_training_stream_and_rng_alone():
    from dedloc_amd.training.evaluation import evaluate

    model = _tiny()
    model.train()

    def make():
        return _stream("fixed", seed=77, B=2)

    runs = []
    for with_eval in (False, True):
        torch.manual_seed(5)
        train = _stream("hf", seed=11)
        train.next_batch()
        if with_eval:
            evaluate(model, make, 2)
        runs.append((train.next_batch(), torch.get_rng_state(), train.gen.get_state()))
    (b0, r0, g0), (b1, r1, g1) = runs
    assert b0.keys() == b1.keys() and all(torch.equal(b0[k], b1[k]) for k in b0)
    assert torch.equal(r0, r1) and torch.equal(g0, g1)


def test_evaluate_is_repeatable_and_consistent():
    from types import SimpleNamespace

    from dedloc_amd.data.synthetic_mlm import peer_seed
    from dedloc_amd.training.evaluation import EVAL_SEED, build_eval_stream, evaluate

    assert EVAL_SEED >= 2 ** 31 > peer_seed(b"any key", 2 ** 40)  # peer_seed is a residue modulo 2**31
    model = _tiny()
    targs = SimpleNamespace(per_device_eval_batch_size=3, seq_length=64)
    dargs = SimpleNamespace(mask_mode="hf", length_mode="wikitext", pattern_period=97, eval_dataset_path=None)

    def make():
        return build_eval_stream(dargs, targs, 512, "cpu")

    s = make()
    assert (s.B, s.S, s.mask_mode, s.length_mode, s.pattern_period) == (3, 64, "hf", "wikitext", 97)
    a, b = evaluate(model, make, 3), evaluate(model, make, 3)
    assert a == b and set(a) == EVAL_KEYS
    assert a["eval_samples"] == 9
    assert a["eval_loss"] == pytest.approx(a["eval_mlm_loss"] + a["eval_sop_loss"], rel=1e-12)
    assert a["eval_perplexity"] == pytest.approx(math.exp(a["eval_mlm_loss"]), rel=1e-12)
    # the sums of evaluate_batch over the same three batches
    st, tot = make(), dict.fromkeys(SUMS, 0.0)
    for _ in range(3):
        out = model.evaluate_batch(st.next_batch())
        for k in SUMS:
            tot[k] += float(out[k])
    assert a["eval_mlm_loss"] == pytest.approx(tot["mlm_loss_sum"] / tot["mlm_count"], rel=1e-9)
    assert a["eval_mlm_accuracy"] == pytest.approx(tot["mlm_top1"] / tot["mlm_count"], rel=1e-9)
    assert a["eval_mlm_top5"] == pytest.approx(tot["mlm_top5"] / tot["mlm_count"], rel=1e-9)
    assert a["eval_sop_accuracy"] == pytest.approx(tot["sop_correct"] / tot["sop_count"], rel=1e-9)
    assert 0.0 <= a["eval_mlm_accuracy"] <= a["eval_mlm_top5"] <= 1.0


def test_build_eval_stream_reads_a_held_out_dataset(tmp_path):
    from types import SimpleNamespace

    from dedloc_amd.data.sop_dataset import DiskSOPStream
    from dedloc_amd.training.evaluation import build_eval_stream, evaluate

    import datasets
    rows = {"input_ids": [[2, 7, 8, 3, 9, 10, 3]] * 5, "token_type_ids": [[0, 0, 0, 0, 1, 1, 1]] * 5,
            "special_tokens_mask": [[1, 0, 0, 1, 0, 0, 1]] * 5, "sentence_order_label": [0, 1, 0, 1, 0]}
    d = tmp_path / "held_out"
    datasets.Dataset.from_dict(rows).save_to_disk(str(d))
    meta = {"cls": 2, "sep": 3, "mask": 4, "pad": 0, "vocab_size": 512, "max_seq_length": 64, "num_instances": 5}
    (d / "sop_meta.json").write_text(json.dumps(meta))

    def make():
        return build_eval_stream(SimpleNamespace(eval_dataset_path=str(d)),
                                 SimpleNamespace(per_device_eval_batch_size=2, seq_length=64), 512, "cpu")

    s = make()
    assert isinstance(s, DiskSOPStream) and s.B == 2
    a, b = s.next_batch(), make().next_batch()  # rebuilt from the fixed seed: the same rows, the same mask
    assert a["input_ids"].shape[0] == 2 and all(torch.equal(a[k], b[k]) for k in a)
    model = _tiny()
    assert evaluate(model, make, 2) == evaluate(model, make, 2)


# ------------------------------------------------------------------ the peer loop
def _run_peer(tmp_path, tag, steps, lr=1.76e-3, **targs_kw):
    from dedloc_amd.cli.arguments import AlbertTrainingArguments, CollaborationArguments, DatasetArguments
    from dedloc_amd.dht import DHT
    from dedloc_amd.models.albert import AlbertConfig
    from dedloc_amd.training.albert_peer import AlbertPeer

    cfg_dir = tmp_path / f"cfg_{tag}"
    AlbertConfig.tiny(num_hidden_layers=2, max_position_embeddings=64).save_pretrained(str(cfg_dir))
    metrics = tmp_path / f"{tag}.jsonl"
    targs = AlbertTrainingArguments(per_device_train_batch_size=16, gradient_accumulation_steps=1, seq_length=64,
                                    warmup_steps=10, max_steps=10 ** 6, learning_rate=lr, save_steps=0,
                                    output_dir=str(tmp_path / f"out_{tag}"), seed=7, metrics_file=str(metrics),
                                    per_device_eval_batch_size=16, **targs_kw)
    dargs = DatasetArguments(config_path=str(cfg_dir), mask_mode="hf", pattern_period=97)
    root = DHT(listen_on="127.0.0.1:*")
    cargs = CollaborationArguments(experiment_prefix=f"eval_{tag}", initial_peers=[root.endpoint],
                                   dht_listen_on="127.0.0.1:*", listen_on="127.0.0.1:*", target_batch_size=32,
                                   min_refresh_period=0.05, default_refresh_period=0.1)
    peer = AlbertPeer(targs, dargs, cargs, torch.device("cpu"))
    try:
        assert peer.data.pattern_period == 97
        peer.train(stop_after_global_steps=steps)
        return [json.loads(x) for x in metrics.read_text().splitlines()], peer.collab_opt.local_step
    finally:
        peer.shutdown()
        root.shutdown()


LEARN_STEPS, LEARN_EVERY, LEARN_LR = 200, 50, 1.5e-2
# half of the measured drop in eval_mlm_loss (1.468) and gain in eval_mlm_accuracy (0.0774): see the test
HALF_DROP, HALF_ACC_GAIN = 0.73, 0.038


@pytest.mark.timeout(300)
def test_peer_evaluates_and_the_held_out_loss_falls(tmp_path):
    """One CPU peer, tiny config, the learnable stream (pattern_period 97), 200 collaborative steps of
    32 samples at learning rate 1.5e-2 (about 25 s), an evaluation (4 batches of 16) every 50 steps.

    Measured on the CPU (the peer's training stream is seeded by its random key, so runs differ a
    little): eval_mlm_loss 5.9589 at step 50 -> 4.4906 at step 200, a drop of 1.468 (a second run:
    5.9591 -> 4.4842); eval_mlm_accuracy 0.0118 -> 0.0892, a gain of 0.0774 (second run: 0.0135 ->
    0.1027).  At the reference learning rate 1.76e-3 the same model moves 6.24 -> 5.80 in 300 steps.
    The test asserts half the measured drop (0.73) and half the measured accuracy gain (0.038)."""
    recs, last_step = _run_peer(tmp_path, "on", LEARN_STEPS, lr=LEARN_LR, do_eval=True, eval_steps=LEARN_EVERY, eval_max_batches=4)
    ev = [r for r in recs if r.get("eval")]
    train = [r for r in recs if not r.get("eval")]
    assert [r["step"] for r in ev] == list(range(LEARN_EVERY, last_step + 1, LEARN_EVERY)) + (
        [last_step] if last_step % LEARN_EVERY else [])
    assert all(EVAL_KEYS <= set(r) and r["eval"] is True and r["eval_samples"] == 64 for r in ev)
    assert train and all("eval_loss" not in r and "loss" in r for r in train)
    first, last = ev[0], ev[-1]
    print(f"eval_mlm_loss {first['eval_mlm_loss']:.4f} -> {last['eval_mlm_loss']:.4f}; "
          f"eval_mlm_accuracy {first['eval_mlm_accuracy']:.4f} -> {last['eval_mlm_accuracy']:.4f}")
    assert last["eval_mlm_loss"] < first["eval_mlm_loss"] - HALF_DROP
    assert last["eval_mlm_accuracy"] > first["eval_mlm_accuracy"] + HALF_ACC_GAIN



@pytest.mark.timeout(300)
def test_peer_without_do_eval_runs_nothing_new(tmp_path):
    recs, _ = _run_peer(tmp_path, "off", 3, eval_steps=1)  # do_eval False: eval_steps alone does nothing
    assert recs and not any("eval" in r or any(k.startswith("eval_") for k in r) for r in recs)
    # the training records' keys are the ones the peer wrote before evaluation existed
    assert {"step", "samples_per_second", "samples_accumulated", "loss", "mini_steps", "time", "hf_step", "lr",
            "group", "matchmaking_s", "allreduce_s", "parts"} <= set(recs[0])
    assert all(set(r) == set(recs[0]) for r in recs)


# ------------------------------------------------------------------ the coordinator
def test_coordinator_evaluates_after_save_state(tmp_path):
    from dedloc_amd.cli.arguments import AveragerArguments, CollaborativeOptimizerArguments, CoordinatorArguments
    from dedloc_amd.cli.run_first_peer import CheckpointHandler, record_step
    from dedloc_amd.dht import DHT
    from dedloc_amd.models.albert import AlbertConfig

    cfg_dir = tmp_path / "cfg"
    AlbertConfig.tiny(num_hidden_layers=2, max_position_embeddings=64).save_pretrained(str(cfg_dir))
    agg = {"step": 1, "loss": 3.25, "alive peers": 1, "samples": 32, "performance": 10.0}
    dht = DHT(start=True)
    try:
        for do_eval in (True, False):
            ca = CoordinatorArguments(experiment_prefix=f"ck{int(do_eval)}", model_config_path=str(cfg_dir),
                                      save_checkpoint_step_interval=1, do_eval=do_eval, eval_max_batches=2)
            h = CheckpointHandler(ca, CollaborativeOptimizerArguments(), AveragerArguments(), dht, b"coord")
            try:
                metrics = tmp_path / f"coord{int(do_eval)}.jsonl"
                rec = record_step(h, agg, True, str(metrics))
                lines = [json.loads(x) for x in metrics.read_text().splitlines()]
                assert lines == [rec] and h.previous_step == 1
                if do_eval:
                    assert EVAL_KEYS <= set(rec) and math.isfinite(rec["eval_loss"]) and rec["eval_samples"] == 8
                    assert rec["eval_loss"] == pytest.approx(h.evaluate()["eval_loss"], rel=0, abs=0)
                else:
                    assert set(rec) == set(agg) | {"time"}
                # a record between saves carries no evaluation
                assert "eval_loss" not in record_step(h, dict(agg, **{"alive peers": 2}), False, str(metrics))
            finally:
                h.collaborative_optimizer.shutdown()
    finally:
        dht.shutdown()


# ------------------------------------------------------------------ GPU against the CPU result
@pytest.mark.gpu
def test_evaluate_batch_gpu_matches_cpu(cuda):
    """Tiny config at hidden_size 128 (head_dim 64), rectangular and packed, against the same
    model's CPU result: exact counts, mean losses within the relative 1e-2 that
    tests/test_albert_packed_gpu.py allows between packed and padded losses."""
    cpu = _tiny()
    gpu = _tiny(device=cuda)
    gpu.load_hf_state_dict(cpu.hf_state_dict())
    assert gpu.config.hidden_size // gpu.config.num_attention_heads == 64
    stream = _stream("hf", length_mode="uniform", min_len=9, B=8)
    batch = stream.next_batch()
    lengths = stream.last_lengths
    want = cpu.evaluate_batch(batch)
    gbatch = {k: v.to(cuda) for k, v in batch.items()}
    for packed in (False, True):
        gpu.pack_sequences = packed
        got = gpu.evaluate_batch(gbatch, lengths=lengths if packed else None)
        assert all(v.is_cuda and v.dim() == 0 for v in got.values())
        margins = {}
        for head in ("mlm", "sop"):
            n = int(want[f"{head}_count"])
            assert int(got[f"{head}_count"]) == n and n > 0
            ref = float(want[f"{head}_loss_sum"]) / n
            margins[head] = abs(float(got[f"{head}_loss_sum"]) / n - ref) / abs(ref)
        print(f"evaluate_batch gpu vs cpu (packed={packed}): relative loss error {margins} (bound 1e-2)")
        record_margin(f"evaluate_batch_gpu_vs_cpu[packed={packed}]", bound=1e-2, **margins)
        assert max(margins.values()) < 1e-2, margins
