"""kNN evaluation, CPU tier: the CPU operators against the fp64 references of tests/knn_checks.py,
the labelled image folder, the evaluation transform, and the evaluation end to end on a tiny folder
(model, streams, peer)."""
import json
import math

import numpy as np
import pytest
import torch

import knn_checks as kc
import dedloc_amd.ops as ops
from dedloc_amd.data.multicrop import MultiCropAugment, augment_reference_ragged
from dedloc_amd.utils.config import load_config

OPS = torch.ops.dedloc


# ------------------------------------------------------------------ operators
@pytest.mark.parametrize("Q,N,D,k", [(1, 5, 16, 5), (33, 257, 24, 200), (7, 1000, 128, 256), (130, 300, 2048, 1),
                                     (0, 9, 16, 3)])
def test_topk_cpu_is_exact_on_exact_inputs(Q, N, D, k):
    q, bank = kc.exact_inputs(Q, N, D, seed=Q + N)
    vals, idx = OPS.knn_topk(q, bank, k, 0)
    assert vals.shape == (Q, k) and vals.dtype == torch.float32 and idx.dtype == torch.int32
    rv, ri = kc.topk_reference(q, bank, k)
    assert torch.equal(idx.long(), ri) and torch.equal(vals.double(), rv)
    if Q:
        s = kc.scores64(q, bank)
        assert (s.sort(1).values[:, 1:] == s.sort(1).values[:, :-1]).any()  # the inputs do hold ties


def test_topk_cpu_ties_and_domain():
    q, bank = kc.exact_inputs(3, 40, 16, seed=1)
    same = bank[:1].repeat(40, 1).contiguous()
    assert torch.equal(OPS.knn_topk(q, same, 7, 0)[1], torch.arange(7, dtype=torch.int32).repeat(3, 1))
    dup = bank[:20].repeat_interleave(2, 0).contiguous()
    idx = OPS.knn_topk(q, dup, 10, 3)[1]
    assert (idx[:, 0::2] % 2 == 0).all() and torch.equal(idx[:, 1::2], idx[:, 0::2] + 1)  # pairs in index order
    for bad_k in (0, 41, 257):
        with pytest.raises(RuntimeError):
            OPS.knn_topk(q, bank, bad_k, 0)
    with pytest.raises(RuntimeError):
        OPS.knn_topk(q, bank.t().contiguous().t(), 3, 0)
    vals, idx = ops.knn_topk(q.float(), bank.float(), 4)  # the wrapper casts
    assert torch.equal(idx, OPS.knn_topk(q, bank, 4, 0)[1])


def test_vote_cpu_hand_cases_and_random():
    vals, idx, labels, targets, C, pred, rank = kc.hand_vote_cases()
    p, r = OPS.knn_vote(vals, idx, labels, targets, C, 0.1)
    assert p.dtype == torch.int32 and r.dtype == torch.int32
    assert p.tolist() == pred and r.tolist() == rank
    assert kc.vote_reference(vals, idx, labels, targets, C, 0.1) == (pred, rank)
    g = torch.Generator().manual_seed(3)
    for C in (1, 7, 50):
        N, Q, k = 300, 40, 20
        labels = torch.randint(-1, C + 1, (N,), generator=g).to(torch.int32)  # -1 and C: out of range
        idx = torch.stack([torch.randperm(N, generator=g)[:k] for _ in range(Q)]).to(torch.int32)
        vals = torch.rand(Q, k, generator=g).sort(1, descending=True).values
        targets = torch.randint(-1, C + 1, (Q,), generator=g)
        p, r = OPS.knn_vote(vals, idx, labels, targets, C, 0.1)
        rp, rr = kc.vote_reference(vals, idx, labels, targets, C, 0.1)
        assert p.tolist() == rp and r.tolist() == rr


def test_classify_counts():
    vals, idx, labels, targets, C, _, rank = kc.hand_vote_cases()
    bank = torch.eye(16)[:6].to(torch.bfloat16)  # bank row i = unit vector i: query i's neighbour 0 is i
    out = ops.knn_classify(bank[:4], bank, labels, torch.tensor([0, 1, 2, 0]), C, k=1)
    assert int(out["count"]) == 4 and int(out["top1"]) == 3 and int(out["top5"]) == 3
    assert out["rank"].tolist() == [0, 0, 0, -1] and out["pred"].tolist() == [0, 1, 2, 1]


# ------------------------------------------------------------------ labelled folder, transform
def test_dataset_labels_and_classes(tmp_path):
    from dedloc_amd.data.image_folder import ImageFolderDataset

    im = np.zeros((4, 5, 3), dtype=np.uint8)
    a, b = tmp_path / "a", tmp_path / "b"
    for p in (a / "dog", a / "cat" / "deep" / "er", b / "bird", b / "cat", b / "empty"):
        p.mkdir(parents=True)
    for p in (a / "top.npy", a / "dog" / "1.npy", a / "cat" / "deep" / "er" / "2.npy", a / "cat" / "3.npy",
              b / "bird" / "4.npy", b / "cat" / "5.npy", b / "6.npy"):
        np.save(p, im)
    ds = ImageFolderDataset([str(a), str(b)])
    assert ds.classes == ["bird", "cat", "dog", "empty"]
    assert ds.labels.dtype == torch.int64 and len(ds.labels) == len(ds.files) == 7
    got = {f[len(str(tmp_path)) + 1:]: int(l) for f, l in zip(ds.files, ds.labels)}
    assert got == {"a/top.npy": -1, "a/dog/1.npy": 2, "a/cat/deep/er/2.npy": 1, "a/cat/3.npy": 1,
                   "b/bird/4.npy": 0, "b/cat/5.npy": 1, "b/6.npy": -1}
    assert ds.files == sorted(ds.files)


@pytest.mark.parametrize("H,W", [(192, 320), (320, 192)])  # landscape, portrait
def test_center_params_against_resize_center_crop(H, W):
    size, resize = 64, 96
    p = MultiCropAugment.center_params(torch.tensor([0]), torch.tensor([H]), torch.tensor([W]), size, resize)
    assert p.shape == (1, 20) and p.dtype == torch.float32
    # Resize(96): the shorter side 192 -> 96 (scale 1/2); CenterCrop(64) cuts [16, 80) of it and the
    # centred 64 of the longer side 160: in source pixels a 128 box at (320 - 128) / 2 = 96 and 32
    side, left, top = 128, (W - 128) // 2, (H - 128) // 2
    assert p[0, :5].tolist() == [0, left, top, side, side]
    ident = torch.zeros(15)
    ident[0:3] = 1.0
    ident[[5, 9, 13]] = 1.0
    assert torch.equal(p[0, 5:], ident)  # colour 1 1 1, apply 0, grey 0, identity matrix, sigma 0
    Image = pytest.importorskip("PIL.Image")
    g = torch.Generator().manual_seed(H)
    low = torch.randint(0, 256, (H // 16, W // 16, 3), generator=g, dtype=torch.uint8)
    img = low.repeat_interleave(16, 0).repeat_interleave(16, 1).contiguous()  # smooth at the filter's scale
    pil = Image.fromarray(img.numpy())
    rw, rh = (resize * W // H, resize) if W >= H else (resize, resize * H // W)
    pil = pil.resize((rw, rh), Image.BILINEAR)
    l, t = round((rw - size) / 2), round((rh - size) / 2)
    ref = torch.from_numpy(np.array(pil.crop((l, t, l + size, t + size)))).permute(2, 0, 1).float() / 255
    aug = MultiCropAugment(mean=(0, 0, 0), std=(1, 1, 1))
    meta = torch.tensor([[0, H, W]], dtype=torch.int64)
    out = augment_reference_ragged(img.reshape(-1), meta, p, size, aug.rad, aug.mean, aug.std)[0].float()
    # one 8-bit rounding of PIL's two passes and one bf16 rounding of a value in [0, 1]; away from the
    # box edge (whose taps PIL fills from outside the box) the two pipelines sample the same pixels
    assert (out - ref)[:, 2:-2, 2:-2].abs().max() <= 2 / 255 + 2 ** -8


# ------------------------------------------------------------------ end to end on a tiny folder
def _image(k, H=40, W=56):
    """Image k of the tiny folder: a solid colour of its own plus a fixed pattern (stripes whose
    period and direction depend on k), so that no two images' features coincide in bf16."""
    colours = [(200, 30, 30), (30, 200, 30), (30, 30, 200), (200, 200, 30), (200, 30, 200), (30, 200, 200),
               (240, 240, 240), (15, 15, 15), (128, 64, 0), (0, 128, 64), (64, 0, 128), (128, 128, 128)]
    yy, xx = np.mgrid[0:H, 0:W]
    wave = ((xx if k % 2 else yy) // (2 + k % 5)) % 2
    img = np.empty((H, W, 3), dtype=np.float32)
    img[:] = colours[k]
    img *= (0.4 + 0.6 * wave)[:, :, None]
    return img.astype(np.uint8)


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """12 images: ``own`` one class per image, ``three`` the same images in 3 classes of 4."""
    root = tmp_path_factory.mktemp("knn")
    for k in range(12):
        for name, cls in (("own", f"c{k:02d}"), ("three", f"g{k % 3}")):
            d = root / name / cls
            d.mkdir(parents=True, exist_ok=True)
            np.save(d / f"{k:02d}.npy", _image(k))
    return root


@pytest.fixture(scope="module")
def model():
    from dedloc_amd.models.resnet_swav import SwAVModel

    torch.manual_seed(0)
    m = SwAVModel(num_prototypes=16)
    m.train()
    return m


def _streams(root, name, batch=5):
    from dedloc_amd.data.image_folder import ImageFolderDataset, ImageFolderEvalStream

    ds = ImageFolderDataset([str(root / name)])
    return [ImageFolderEvalStream(ds, batch, "cpu", size=64, resize=72, num_workers=2) for _ in range(2)]


def test_eval_stream_serves_every_image_once_in_order(tiny):
    (s, _) = _streams(tiny, "own")
    shapes, labels = [], []
    for x, y in s:
        assert x.dtype == torch.bfloat16 and x.is_contiguous(memory_format=torch.channels_last)
        shapes.append(tuple(x.shape))
        labels += y.tolist()
    assert shapes == [(5, 3, 64, 64), (5, 3, 64, 64), (2, 3, 64, 64)] and labels == list(range(12))
    assert [y.tolist() for _, y in s][0] == [0, 1, 2, 3, 4]  # a second pass starts over


def test_knn_evaluate_end_to_end(tiny, model):
    from dedloc_amd.training.swav_eval import extract_features, knn_evaluate

    before = {k: v.clone() for k, v in model.state_dict().items()}
    bank, query = _streams(tiny, "own")
    out = knn_evaluate(model, bank, query, k=1)
    assert out == {"knn_top1": 1.0, "knn_top5": 1.0, "knn_samples": 12, "knn_bank": 12, "knn_k": 1}
    assert model.training
    after = model.state_dict()
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    for feature, D in (("trunk", 2048), ("head", 128)):
        bank, query = _streams(tiny, "three")
        f, y = extract_features(model, bank, feature)
        assert f.shape == (12, D) and f.dtype == torch.bfloat16 and y.tolist() == [k // 4 for k in range(12)]  # files sort by class directory
        assert (f.float().norm(dim=1) - 1).abs().max() < 2 ** -7
        out = knn_evaluate(model, bank, query, k=200, sigma=0.1, feature=feature)  # k is cut to the bank: 12
        rv, ri = kc.topk_reference(f, f, 12)
        _, rank = kc.vote_reference(rv, ri, y, y, 3, 0.1)
        assert out["knn_k"] == 12 and out["knn_samples"] == 12 and out["knn_bank"] == 12
        assert out["knn_top1"] == sum(r == 0 for r in rank) / 12
        assert out["knn_top5"] == sum(0 <= r < 5 for r in rank) / 12
    model.eval()
    extract_features(model, _streams(tiny, "own")[0])
    assert not model.training
    model.train()
    with pytest.raises(ValueError):
        extract_features(model, _streams(tiny, "own")[0], feature="pool5")
    assert model.training


# ------------------------------------------------------------------ peer and CLI
def _peer_cfg(tmp_path, tiny, extra=()):
    return load_config("swav_1node_resnet_submit", [
        "config.DATA.TRAIN.BATCHSIZE_PER_REPLICA=2", "config.DATA.TRAIN.MULTICROP.size_crops=[32,16]",
        "config.DATA.TRAIN.MULTICROP.num_crops=[2,2]", "config.MODEL.HEAD.num_clusters=16",
        "config.LOSS.swav_loss.queue.queue_length=4", "config.LOSS.swav_loss.queue.start_iter=0",
        "config.OPTIMIZER.target_batch_size=4", "config.OPTIMIZER.batch_size_for_tracking=2",
        "config.OPTIMIZER.warmup_epochs=2", "config.OPTIMIZER.max_epochs=10",
        "config.DATA.TRAIN.DATA_SOURCES=[disk_folder]", f'+config.DATA.TRAIN.DATA_PATHS=["{tiny / "three"}"]',
        f"config.CHECKPOINT.DIR={tmp_path}", f"config.METRICS_FILE={tmp_path / 'metrics.jsonl'}", *extra])


_KNN = ("+config.NEAREST_NEIGHBOR.EVAL_FREQUENCY=1", "+config.NEAREST_NEIGHBOR.CENTER_CROP=64",
        "+config.NEAREST_NEIGHBOR.RESIZE=72", "+config.NEAREST_NEIGHBOR.MAX_BANK_IMAGES=9",
        "+config.NEAREST_NEIGHBOR.TOPK=3", "+config.DATA.TEST.DATA_SOURCES=[disk_folder]")


def _run_peer(cfg, steps):
    from dedloc_amd.dht import DHT
    from dedloc_amd.training.swav_peer import SwavPeer

    dht = DHT(start=True)
    peer = SwavPeer(cfg, "cpu", dht=dht)
    try:
        peer.train(max_iterations=steps)
        return peer
    finally:
        peer.shutdown()
        dht.shutdown()


def test_swav_peer_cpu_appends_eval_lines(tmp_path, tiny):
    cfg = _peer_cfg(tmp_path, tiny, _KNN + (f'+config.DATA.TEST.DATA_PATHS=["{tiny / "three"}"]',))
    peer = _run_peer(cfg, 4)
    assert len(peer.knn["bank_indices"]) == 9 and len(peer.knn["query_indices"]) == 12
    lines = [json.loads(l) for l in open(cfg.METRICS_FILE)]
    evals = [l for l in lines if l.get("eval")]
    assert evals and len(lines) > len(evals)
    for l in evals:
        assert l["eval"] is True and {"knn_top1", "knn_top5", "knn_samples", "knn_bank", "knn_k", "step"} <= set(l)
        assert l["knn_samples"] == 12 and l["knn_bank"] == 9 and l["knn_k"] == 3
        assert 0.0 <= l["knn_top1"] <= l["knn_top5"] <= 1.0
    assert lines[-1].get("eval")  # train() ends on an evaluation
    steps = [l["step"] for l in evals]
    assert steps == sorted(set(steps))  # one evaluation per global step


def test_swav_peer_without_the_key_writes_todays_lines(tmp_path, tiny):
    peer = _run_peer(_peer_cfg(tmp_path, tiny), 4)
    assert peer.knn is None
    lines = [json.loads(l) for l in open(peer.cfg.METRICS_FILE)]
    assert lines and lines == [json.loads(json.dumps(r)) for r in peer.metrics_log]
    for l in lines:
        assert "eval" not in l and not any(k.startswith("knn_") for k in l)
        assert {"step", "samples_per_second", "samples_accumulated", "loss", "mini_steps", "time", "iteration", "lr",
                "queue"} <= set(l)
        assert math.isfinite(l["loss"])


def test_swav_peer_rejects_evaluation_without_labels(tmp_path, tiny):
    from dedloc_amd.training.swav_peer import SwavPeer

    test_paths = f'+config.DATA.TEST.DATA_PATHS=["{tiny / "three"}"]'
    synthetic = _peer_cfg(tmp_path, tiny, _KNN + (test_paths, "config.DATA.TRAIN.DATA_SOURCES=[synthetic]"))
    with pytest.raises(ValueError, match="disk_folder"):
        SwavPeer(synthetic, "cpu")
    with pytest.raises(ValueError, match="DATA.TEST"):
        SwavPeer(_peer_cfg(tmp_path, tiny, _KNN), "cpu")
    flat = tmp_path / "flat"
    flat.mkdir()
    np.save(flat / "0.npy", _image(0))
    with pytest.raises(ValueError, match="no labelled file"):
        SwavPeer(_peer_cfg(tmp_path, tiny, _KNN + (test_paths, f'+config.NEAREST_NEIGHBOR.BANK_PATHS=["{flat}"]')),
                 "cpu")


def test_knn_swav_cli_prints_one_json_line(tmp_path, tiny, model, capsys):
    from dedloc_amd.cli import knn_swav

    ckpt = tmp_path / "model.torch"
    torch.save({"model": {k: v.detach().cpu() for k, v in model.state_dict().items()}, "iteration": 7,
                "collab_step": 2}, ckpt)
    out = knn_swav.main([
        "config=pretrain/swav/swav_1node_resnet_submit", f"+config.CHECKPOINT.PATH={ckpt}",
        "config.MODEL.HEAD.num_clusters=16", f'+config.DATA.TRAIN.DATA_PATHS=["{tiny / "own"}"]',
        "+config.DATA.TEST.DATA_SOURCES=[disk_folder]", f'+config.DATA.TEST.DATA_PATHS=["{tiny / "own"}"]',
        "+config.NEAREST_NEIGHBOR.CENTER_CROP=64", "+config.NEAREST_NEIGHBOR.RESIZE=72",
        "+config.NEAREST_NEIGHBOR.TOPK=1", "--device", "cpu"])
    printed = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(printed) == 1 and json.loads(printed[0]) == out
    assert out["knn_top1"] == 1.0 and out["knn_samples"] == 12 and out["iteration"] == 7 and out["step"] == 2
