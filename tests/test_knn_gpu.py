"""kNN evaluation on the GPU (knn.hip: knn_topk_kernel, knn_merge_kernel, knn_vote_kernel) against the
fp64 references of tests/knn_checks.py, at the smallest shapes at which the kernels can go wrong:
partial query and bank tiles, one and several bank slices, every prune path, ties."""
import math

import numpy as np
import pytest
import torch

import knn_checks as kc
import dedloc_amd.ops  # noqa: F401
from dedloc_amd.data.multicrop import MultiCropAugment, augment_reference_ragged
from dedloc_amd.utils.config import load_config

pytestmark = pytest.mark.gpu
OPS = torch.ops.dedloc


def _topk(q, bank, k, splits, dev):
    vals, idx = OPS.knn_topk(q.to(dev), bank.to(dev), k, splits)
    assert vals.shape == (q.shape[0], k) and vals.dtype == torch.float32 and idx.dtype == torch.int32
    return vals.cpu(), idx.cpu()


# every value of every axis: Q in {1, 31, 33, 64, 130}, N in {k, k + 1, 257, 1000}, D in {16, 128, 2048},
# k in {1, 5, 200, 256}; splits 1 and more
EXACT = [(1, 200, 16, 200, 1), (130, 1000, 128, 200, 1), (130, 1000, 2048, 5, 2), (31, 257, 128, 256, 1),
         (33, 6, 16, 5, 1), (64, 257, 2048, 1, 2), (64, 1, 16, 1, 1), (33, 256, 128, 256, 1), (31, 1000, 16, 256, 3),
         (1, 201, 2048, 200, 2), (0, 50, 16, 5, 1)]


@pytest.mark.parametrize("Q,N,D,k,splits", EXACT)
def test_topk_is_exact_on_exact_inputs(cuda, Q, N, D, k, splits):
    q, bank = kc.exact_inputs(Q, N, D, seed=Q * 7 + N)
    vals, idx = _topk(q, bank, k, splits, cuda)
    rv, ri = kc.topk_reference(q, bank, k)
    assert torch.equal(idx.long(), ri) and torch.equal(vals.double(), rv)


def test_splits_agree_bitwise(cuda):
    q, bank = kc.exact_inputs(130, 1000, 128, seed=2)
    rv, ri = kc.topk_reference(q, bank, 200)
    for splits in (1, 2, 7):  # 7 does not divide 1000
        vals, idx = _topk(q, bank, 200, splits, cuda)
        assert torch.equal(idx.long(), ri) and torch.equal(vals.double(), rv), splits
    # the automatic choice where it is more than one slice: one query tile and 4096 bank rows give
    # min(2 CUs, 4096 / 512, 32) = 8 slices on any device with 4 CUs or more (dl_knn_splits)
    q, bank = kc.exact_inputs(64, 4096, 16, seed=3)
    one, auto = _topk(q, bank, 5, 1, cuda), _topk(q, bank, 5, 0, cuda)
    rv, ri = kc.topk_reference(q, bank, 5)
    assert torch.equal(one[0], auto[0]) and torch.equal(one[1], auto[1])
    assert torch.equal(auto[1].long(), ri) and torch.equal(auto[0].double(), rv)


@pytest.mark.parametrize("order", ["ascending", "descending", "random"])
def test_order_adversaries(cuda, order):
    """Ascending: every tile's entries survive (a prune per tile); descending: nothing survives
    after the first tiles; one fixed permutation."""
    q, bank = kc.order_adversary(2000, 16, order, seed=4)
    q = q.repeat(3, 1).contiguous()
    for k, splits in ((200, 1), (200, 3), (1, 1), (256, 2)):
        vals, idx = _topk(q, bank, k, splits, cuda)
        rv, ri = kc.topk_reference(q, bank, k)
        assert torch.equal(idx.long(), ri) and torch.equal(vals.double(), rv), (k, splits)
        assert vals[0].tolist() == list(range(1999, 1999 - k, -1))


def test_ties_resolve_to_the_lower_index(cuda):
    q, bank = kc.exact_inputs(5, 150, 16, seed=5)
    same = bank[:1].repeat(300, 1).contiguous()
    for splits in (1, 2):
        assert torch.equal(_topk(q, same, 256, splits, cuda)[1], torch.arange(256, dtype=torch.int32).repeat(5, 1))
    dup = bank.repeat_interleave(2, 0).contiguous()  # every bank row twice
    for splits in (1, 3):
        vals, idx = _topk(q, dup, 200, splits, cuda)
        assert (idx[:, 0::2] % 2 == 0).all() and torch.equal(idx[:, 1::2], idx[:, 0::2] + 1)
        assert torch.equal(idx.long(), kc.topk_reference(q, dup, 200)[1])


@pytest.mark.parametrize("D", [128, 2048])
def test_random_features_within_the_fp32_bound(cuda, D):
    """fp32 accumulation of D exact bf16 products in any order is within D * 2^-24 * sum_d |q_d b_d| of
    the fp64 score; a returned index may therefore trail the true k-th score by at most that."""
    g = torch.Generator().manual_seed(D)
    Q, N, k = 33, 1000, 200
    q, bank = torch.randn(Q, D, generator=g).to(torch.bfloat16), torch.randn(N, D, generator=g).to(torch.bfloat16)
    s = kc.scores64(q, bank)
    bound = D * 2.0 ** -24 * (q.double().abs() @ bank.double().abs().t())
    kth = s.sort(1, descending=True).values[:, k - 1:k]
    for splits in (1, 2):
        vals, idx = _topk(q, bank, k, splits, cuda)
        i = idx.long()
        assert ((i >= 0) & (i < N)).all() and all(len(set(r)) == k for r in i.tolist())
        err = (vals.double() - s.gather(1, i)).abs()
        print(f"knn_topk D={D} splits={splits}: max err / bound {(err / bound.gather(1, i)).max():.4f}")
        assert (err <= bound.gather(1, i)).all()
        assert (s.gather(1, i) >= kth - bound.gather(1, i)).all()
        assert (vals[:, 1:] <= vals[:, :-1]).all()
        again = _topk(q, bank, k, splits, cuda)
        assert torch.equal(again[0], vals) and torch.equal(again[1], idx)  # bitwise, run to run


def test_domain_errors_raise(cuda):
    q, bank = (t.to(cuda) for t in kc.exact_inputs(4, 40, 32, seed=6))
    with pytest.raises(RuntimeError, match="k = 41"):
        OPS.knn_topk(q, bank, 41, 1)
    with pytest.raises(RuntimeError, match="k = 257"):
        OPS.knn_topk(q, bank.repeat(8, 1), 257, 1)
    with pytest.raises(RuntimeError, match="k = 0"):
        OPS.knn_topk(q, bank, 0, 1)
    with pytest.raises(RuntimeError, match="D = 24"):
        OPS.knn_topk(q[:, :24].contiguous(), bank[:, :24].contiguous(), 3, 1)
    with pytest.raises(RuntimeError, match="contiguous"):
        OPS.knn_topk(q[:, :16], bank[:, :16], 3, 1)
    with pytest.raises(RuntimeError, match="splits"):
        OPS.knn_topk(q, bank, 3, 33)
    with pytest.raises(RuntimeError):
        OPS.knn_topk(q.float(), bank, 3, 1)
    vals = torch.zeros(2, 3, device=cuda)
    idx = torch.zeros(2, 3, dtype=torch.int32, device=cuda)
    labels, targets = torch.zeros(5, dtype=torch.int32, device=cuda), torch.zeros(2, dtype=torch.int64, device=cuda)
    for C in (0, 8193):
        with pytest.raises(RuntimeError, match="num_classes"):
            OPS.knn_vote(vals, idx, labels, targets, C, 0.1)
    with pytest.raises(RuntimeError):
        OPS.knn_vote(vals, idx.long(), labels, targets, 3, 0.1)
    torch.cuda.synchronize()


def test_vote_equals_the_cpu_op(cuda):
    def both(vals, idx, labels, targets, C):
        p, r = OPS.knn_vote(vals.to(cuda), idx.to(cuda), labels.to(cuda), targets.to(cuda), C, 0.1)
        cp, cr = OPS.knn_vote(vals, idx, labels, targets, C, 0.1)
        assert p.dtype == torch.int32 and r.dtype == torch.int32
        assert torch.equal(p.cpu(), cp) and torch.equal(r.cpu(), cr)
        return p.cpu().tolist(), r.cpu().tolist()

    vals, idx, labels, targets, C, pred, rank = kc.hand_vote_cases()
    assert both(vals, idx, labels, targets, C) == (pred, rank)
    g = torch.Generator().manual_seed(7)
    for C, k in ((1, 5), (7, 200), (1000, 256)):
        N, Q = 3000, 70
        labels = torch.randint(-1, C + 1, (N,), generator=g).to(torch.int32)  # -1 and C: out of range
        idx = torch.stack([torch.randperm(N, generator=g)[:k] for _ in range(Q)]).to(torch.int32)
        vals = torch.rand(Q, k, generator=g).sort(1, descending=True).values
        targets = torch.randint(-1, C + 1, (Q,), generator=g)
        both(vals, idx, labels, targets, C)


# ------------------------------------------------------------------ transform, features, peer
def test_eval_transform_matches_the_cpu_op(cuda):
    sizes = [(40, 56), (300, 260), (64, 64), (129, 257), (7, 5)]
    g = torch.Generator().manual_seed(8)
    images = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for h, w in sizes]
    off = np.cumsum([0] + [im.numel() for im in images[:-1]])
    meta = torch.tensor([[int(o), h, w] for o, (h, w) in zip(off, sizes)], dtype=torch.int64)
    data = torch.cat([im.reshape(-1) for im in images])
    aug = MultiCropAugment()
    for size, resize in ((64, 72), (224, 256)):
        p = aug.center_params(torch.arange(len(sizes)), meta[:, 1], meta[:, 2], size, resize)
        ref = augment_reference_ragged(data, meta, p, size, aug.rad, aug.mean, aug.std).float()
        out = OPS.multicrop_ragged(data.to(cuda), meta.to(cuda), p.to(cuda), size, aug.rad, list(aug.mean),
                                   list(aug.std)).cpu().float()
        err = (out - ref).abs()
        print(f"eval transform S={size}: max {err.max():.6f} mean {err.mean():.7f}")
        # tests/test_multicrop_ragged_gpu.py: the kernel's geometry-only bound (its measured maximum
        # plus one bf16 step at the output's magnitude) and the pipeline's mean bound
        assert err.max() <= 0.015625 + 2.0 ** -6 and err.mean() < 2e-3


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    root = tmp_path_factory.mktemp("knn_images")
    g = torch.Generator().manual_seed(9)
    for k, (h, w) in enumerate([(40, 56), (64, 64), (33, 91), (75, 50), (48, 48), (101, 37), (57, 57), (80, 120)]):
        d = root / f"class{k % 2}"
        d.mkdir(exist_ok=True)
        np.save(d / f"{k}.npy", torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).numpy())
    return root


def test_extract_features_leaves_the_model_alone(cuda, folder):
    from dedloc_amd.data.image_folder import ImageFolderDataset, ImageFolderEvalStream
    from dedloc_amd.models.resnet_swav import SwAVModel
    from dedloc_amd.training.swav_eval import extract_features, knn_evaluate

    torch.manual_seed(0)
    model = SwAVModel(num_prototypes=16).to(cuda)
    model.train()
    with torch.no_grad():  # running statistics that are not the initial 0 / 1
        for m in model.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.running_mean.uniform_(-0.1, 0.1)
                m.running_var.uniform_(0.8, 1.2)
                m.num_batches_tracked.fill_(3)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    ds = ImageFolderDataset([str(folder)])
    streams = [ImageFolderEvalStream(ds, 3, cuda, size=64, resize=72, num_workers=2) for _ in range(2)]
    f, y = extract_features(model, streams[0])
    assert f.is_cuda and f.shape == (8, 2048) and f.dtype == torch.bfloat16
    assert y.tolist() == [0, 0, 0, 0, 1, 1, 1, 1] and (f.float().norm(dim=1) - 1).abs().max() < 2 ** -7
    h, _ = extract_features(model, streams[0], "head")
    assert h.shape == (8, 128)
    out = knn_evaluate(model, streams[0], streams[1], k=200)
    assert out["knn_k"] == 8 and out["knn_samples"] == 8 and out["knn_bank"] == 8
    rv, ri = kc.topk_reference(f, f, 8)
    _, rank = kc.vote_reference(rv, ri, y, y, 2, 0.1)
    assert out["knn_top1"] == sum(r == 0 for r in rank) / 8 and out["knn_top5"] == 1.0
    assert model.training
    after = model.state_dict()
    assert before.keys() == after.keys()
    for k in before:  # parameters, running_mean / running_var, num_batches_tracked
        assert torch.equal(before[k], after[k]), k
    for s in streams:
        s.close()


def test_train_step_after_an_evaluation_equals_the_step_without(cuda, folder, tmp_path, monkeypatch):
    """Two peers from one seed take one step on the same crops, one of them after an evaluation.
    The step's forward (embeddings and scores over all crops) is equal bit for bit;
    DEDLOC_DETERMINISTIC_BN makes the BatchNorm statistics (fp32 atomics otherwise) reproducible so
    that it can be.  The loss scalar itself is not reproducible run to run, evaluation or not:
    swav.hip adds the 32 per-(crop, row) terms with one float atomic each, in arrival order (measured
    on an MI355X: 2.920487880706787 against 2.920488119125366, one fp32 step, from forwards equal
    bit for bit).  The terms are cross-entropies, all >= 0, so any two orders of the fp32 sum lie
    within (32 - 1) * 2^-24 * loss of each other: the losses are held to that."""
    from dedloc_amd.dht import DHT
    from dedloc_amd.training.swav_peer import SwavPeer

    monkeypatch.setenv("DEDLOC_DETERMINISTIC_BN", "1")
    losses, forwards = [], []
    crops = None
    for evaluate in (True, False):
        cfg = load_config("swav_1node_resnet_submit", [
            "config.DATA.TRAIN.BATCHSIZE_PER_REPLICA=4", "config.DATA.TRAIN.MULTICROP.size_crops=[32,16]",
            "config.DATA.TRAIN.DATA_SOURCES=[disk_folder]", f'+config.DATA.TRAIN.DATA_PATHS=["{folder}"]',
            "config.LOSS.swav_loss.queue.start_iter=0", "config.LOSS.swav_loss.queue.queue_length=64",
            "config.OPTIMIZER.target_batch_size=8", "config.OPTIMIZER.batch_size_for_tracking=4",
            "config.MODEL.HEAD.num_clusters=16", f"config.CHECKPOINT.DIR={tmp_path}", "config.MODEL.CUDA_GRAPH=false",
            "+config.NEAREST_NEIGHBOR.EVAL_FREQUENCY=1000", "+config.NEAREST_NEIGHBOR.CENTER_CROP=64",
            "+config.NEAREST_NEIGHBOR.RESIZE=72", "+config.DATA.TEST.DATA_SOURCES=[disk_folder]",
            f'+config.DATA.TEST.DATA_PATHS=["{folder}"]'])
        dht = DHT(start=True)
        peer = SwavPeer(cfg, cuda, dht=dht)
        try:
            if crops is None:
                crops = [c.clone() for c in peer.data.next_batch()]
            if evaluate:
                rec = peer.evaluate()
                assert rec["eval"] is True and rec["knn_samples"] == 8 and rec["knn_bank"] == 8 and rec["knn_k"] == 8
            inner = peer._forward

            def recording(c, inner=inner):
                emb, scores = inner(c)
                forwards.append((emb.detach().clone(), scores.detach().clone()))
                return emb, scores

            peer._forward = recording
            losses.append(float(peer.train_step([c.clone() for c in crops])))
        finally:
            peer.shutdown()
            dht.shutdown()
    print(f"loss after an evaluation {losses[0]!r}, without {losses[1]!r}")
    (emb_a, scores_a), (emb_b, scores_b) = forwards
    assert emb_a.shape[0] == 8 * 4 and torch.equal(emb_a, emb_b) and torch.equal(scores_a, scores_b)
    assert math.isfinite(losses[0]) and abs(losses[0] - losses[1]) <= 31 * 2.0 ** -24 * abs(losses[1])
